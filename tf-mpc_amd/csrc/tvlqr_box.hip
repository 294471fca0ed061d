// tvlqr_box.hip -- control-limited TIME-VARYING LQR, the forward solve (tfmpc_tvlqr_box_solve_f32):
//   min sum_t 1/2 z_t^T C_t z_t + c_t^T z_t + final cost,  x_{t+1} = F_t z_t + f_t,  low_t <= u_t <= high_t,
// a convex QP with an exact model, solved by control-limited Newton sweeps WITHOUT regularisation.  One wavefront per
// instance, fp32, the LDS layout and per-step model copy of tvlqr_wave.h's fp32 policy, products on the f32 matrix cores.
//
// Per pass: a backward sweep in delta form around the nominal (x, u) -- Q = C_t + F_t^T V F_t, q = C_t z_t + c_t +
// F_t^T v, a box-QP in du by projected Newton (lane r owns control r; the free block is eliminated without pivoting from
// the augmented [Q_uu | g | Q_ux] with held rows and columns replaced by identity, so ONE elimination gives the Newton
// step and the gains K_f), V <- sym(Q_xx + Q_xu K), v <- q_x + Q_xu k -- then a line search over eleven step sizes, each
// a clipped closed-loop rollout into the workspace; the accepted candidate is copied into the output arrays, which hold
// the nominal.  The sweep that meets the stop rule still has its step applied (in full, untested): a step of tol left out
// is several fp32 roundings of the optimum.  Instances never talk to each other: no atomics, no waits, every loop has a
// fixed bound, and every branch around a fence is taken on a wave-uniform value (a reduction, a ballot or a broadcast).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tvlqr_wave.h"

namespace tfmpc {

namespace {

constexpr int kQpIterations = 100, kQpBacktracks = 21, kAlphas = 11, kTrustedInARow = 3;
constexpr float kArmijo = 1e-4f, kTrustRatio = 1e-6f, kDefaultTol = 4e-6f;
constexpr int kDefaultPasses = 100;
constexpr int kReasonConverged = 0, kReasonNoDecrease = 1, kReasonPassCap = 2, kReasonFailed = 3;

struct TvBoxArgs {
    TvLqrArgs a;                    // model, x0; K, k: the gains (workspace); states, actions, costs: the nominal
    const float *low, *high;        // [m] per (b, t)
    long slow_b, slow_t, shigh_b, shigh_t;
    const float *u_init;            // [T][m] per instance (batch stride su_b) or NULL: zeros
    long su_b;
    int max_iter;
    float tol;
    float *cx, *cu, *cc;            // the candidate trajectory [B][T+1][n], [B][T][m], [B][T+1] (workspace)
    int32_t *iterations, *reason;
    uint32_t *clamp_mask;           // [B][T] or NULL
};

__global__ __launch_bounds__(kWave) void tvlqr_box_solve_kernel(TvBoxArgs p)
{
    extern __shared__ float smem[];
    const TvLqrArgs &a = p.a;
    const int b = blockIdx.x;
    const int lane = lane_id();
    const int n = a.n, m = a.m, d = n + m, T = a.T;
    TvSmem<float> s = tv_carve<false>(smem, n, m);
    const int ldd = s.ldd, ldn = s.ldn, lda = s.lda, ldv = s.ldv;
    const bool own = lane < m;                                   // lane r owns control r (m <= 32)
    const uint32_t all_held = m == 32 ? 0xFFFFFFFFu : ((1u << m) - 1u);

    const float *Cf = a.Cfin ? a.Cfin + (size_t)b * a.sCfin_b : tv_at(a.C, a.sC_b, a.sC_t, b, T - 1);
    const float *cf = a.Cfin ? a.cfin + (size_t)b * a.scfin_b : tv_at(a.c, a.sc_b, a.sc_t, b, T - 1);
    const int ldf = a.Cfin ? n : d;

    const size_t nx = ((size_t)T + 1) * n, nu = (size_t)T * m, nc = (size_t)T + 1;   // one instance's trajectory
    float *xs = a.states + b * nx;
    float *us = a.actions + b * nu;
    float *cs = a.costs + b * nc;
    float *cx = p.cx + b * nx;
    float *cu = p.cu + b * nu;
    float *cc = p.cc + b * nc;
    float *Kg = a.K + (size_t)b * a.sK;
    float *kg = a.k + (size_t)b * a.sk;
    uint32_t *maskg = p.clamp_mask ? p.clamp_mask + (size_t)b * T : nullptr;

    auto load_model = [&](int t, bool with_f) {
        load_matrix(s.F, ldd, tv_at(a.F, a.sF_b, a.sF_t, b, t), n, d);
        load_matrix(s.C, ldd, tv_at(a.C, a.sC_b, a.sC_t, b, t), d, d);
        const float *cg = tv_at(a.c, a.sc_b, a.sc_t, b, t);
        for (int i = lane; i < d; i += kWave) s.c[i] = cg[i];
        if (with_f) {
            const float *fg = tv_at(a.f, a.sf_b, a.sf_t, b, t);
            for (int i = lane; i < n; i += kWave) s.f[i] = fg[i];
        }
    };

    // A rollout from x0 into (ox, ou, oc); returns the total cost, summed in time order.
    //   INIT : u_t = clip(u_init_t or 0); any_free becomes true iff some low != high.
    //   else : u_t = clip(nominal u_t + alpha k_t + K_t (x_t - nominal x_t)) with the gains of the last sweep.
    bool any_free = false;
    auto rollout = [&](const float alpha, const bool init, float *ox, float *ou, float *oc) -> float {
        for (int i = lane; i < n; i += kWave) {
            const float x = a.x0[(size_t)b * n + i];
            s.z[i] = x;
            ox[i] = x;
        }
        float J = 0.0f;
        int loose = 0;
        for (int t = 0; t < T; ++t) {
            load_model(t, true);
            if (!init) {
                load_matrix(s.K, ldn, Kg + (size_t)t * m * n, m, n);
                for (int r = lane; r < m; r += kWave) s.k[r] = kg[(size_t)t * m + r];
                for (int i = lane; i < n; i += kWave) s.q[i] = s.z[i] - xs[(size_t)t * n + i];
            }
            wsync();
            if (own) {
                const float lo = tv_at(p.low, p.slow_b, p.slow_t, b, t)[lane];
                const float hi = tv_at(p.high, p.shigh_b, p.shigh_t, b, t)[lane];
                float u;
                if (init) {
                    u = p.u_init ? p.u_init[(size_t)b * p.su_b + (size_t)t * m + lane] : 0.0f;
                    loose |= lo != hi;
                } else {
                    float fb = 0.0f;
                    for (int j = 0; j < n; ++j) fb = fmaf(s.K[lane * ldn + j], s.q[j], fb);
                    u = fmaf(alpha, s.k[lane], us[(size_t)t * m + lane]) + fb;
                }
                u = fminf(fmaxf(u, lo), hi);
                s.z[n + lane] = u;
                ou[(size_t)t * m + lane] = u;
            }
            wsync();
            float part = 0.0f;                                 // 1/2 z^T C_t z + c_t^T z
            for (int r = lane; r < d; r += kWave) {
                float cz = 0.0f;
                for (int j = 0; j < d; ++j) cz = fmaf(s.C[r * ldd + j], s.z[j], cz);
                part += s.z[r] * (0.5f * cz + s.c[r]);
            }
            for (int i = lane; i < n; i += kWave) {            // x' = F_t z + f_t
                float x = s.f[i];
                for (int j = 0; j < d; ++j) x = fmaf(s.F[i * ldd + j], s.z[j], x);
                s.xn[i] = x;
            }
            const float cost = wave_sum(part);
            if (lane == 0) oc[t] = cost;
            if (init && maskg && lane == 0) maskg[t] = 0u;
            J += cost;
            wsync();
            for (int i = lane; i < n; i += kWave) {
                const float x = s.xn[i];
                s.z[i] = x;
                ox[(size_t)(t + 1) * n + i] = x;
            }
            wsync();
        }
        float part = 0.0f;                                     // 1/2 x^T C_fin x + c_fin^T x
        for (int r = lane; r < n; r += kWave) {
            float cz = 0.0f;
            for (int j = 0; j < n; ++j) cz = fmaf(Cf[r * ldf + j], s.z[j], cz);
            part += s.z[r] * (0.5f * cz + cf[r]);
        }
        const float last = wave_sum(part);
        if (lane == 0) oc[T] = last;
        if (init) any_free = __ballot(loose != 0) != 0;
        return J + last;
    };

    // One backward sweep around the nominal in (xs, us): gains into (Kg, kg), the held sets into maskg.  Returns the
    // sweep's status bits; kmax = max |k|, umax = max |u|, dV = sum k^T q_u + 1/2 k^T Q_uu k.
    auto sweep = [&](float &kmax, float &umax, float &dV) -> int {
        int st = 0;
        float kpart = 0.0f, upart = 0.0f;
        dV = 0.0f;
        kmax = umax = 0.0f;
        wave_for_2d(n, n, [&](int i, int j, int) { s.V[i * ldn + j] = Cf[i * ldf + j]; });
        for (int i = lane; i < n; i += kWave) {                 // v = C_fin x_T + c_fin
            float x = cf[i];
            for (int j = 0; j < n; ++j) x = fmaf(Cf[i * ldf + j], xs[(size_t)T * n + j], x);
            s.v[i] = x;
        }
        wsync();
        for (int t = T - 1; t >= 0; --t) {
            load_model(t, false);
            for (int i = lane; i < n; i += kWave) s.z[i] = xs[(size_t)t * n + i];
            if (own) s.z[n + lane] = us[(size_t)t * m + lane];
            wsync();
            // W = F_t^T V  [d][n]
            wave_matmul_mfma(d, n, n,
                             [&](int r, int k) { return s.F[k * ldd + r]; },
                             [&](int k, int j) { return s.V[k * ldn + j]; },
                             [](int, int) { return 0.0f; },
                             [&](int r, int j, float x) { s.W[r * ldn + j] = x; });
            wsync();
            // Q = C_t + W F_t ; q = C_t z_t + c_t + F_t^T v
            wave_matmul_mfma(d, d, n,
                             [&](int r, int k) { return s.W[r * ldn + k]; },
                             [&](int k, int j) { return s.F[k * ldd + j]; },
                             [&](int r, int j) { return s.C[r * ldd + j]; },
                             [&](int r, int j, float x) { s.Q[r * ldd + j] = x; });
            for (int r = lane; r < d; r += kWave) {
                float s1 = 0.0f, s2 = 0.0f;
                for (int j = 0; j < d; ++j) s1 = fmaf(s.C[r * ldd + j], s.z[j], s1);
                for (int k = 0; k < n; ++k) s2 = fmaf(s.F[k * ldd + r], s.v[k], s2);
                s.q[r] = s.c[r] + s1 + s2;
            }
            wsync();

            // ---- box-QP: min 1/2 x^T Q_uu x + q_u^T x, lo <= x <= hi, from x = 0 (projected Newton) ----
            const float *Quu = s.Q + n * ldd + n;
            float *xv = s.k, *gv = s.prow, *dv = s.z + n;       // x, gradient and trial move, shared through LDS
            const float ub = own ? s.z[n + lane] : 0.0f;
            const float lo = own ? tv_at(p.low, p.slow_b, p.slow_t, b, t)[lane] - ub : 0.0f;
            const float hi = own ? tv_at(p.high, p.shigh_b, p.shigh_t, b, t)[lane] - ub : 0.0f;
            upart = fmaxf(upart, fabsf(ub));
            float x = 0.0f;
            uint32_t held = 0, prev = 0;
            bool full = false;
            int qp = TFMPC_ST_QP_MAXITER;
            wsync();                                            // ub is read before dv (over z_u) is written
            if (own) xv[lane] = 0.0f;
            wsync();
            for (int it = 0; it < kQpIterations; ++it) {
                float g = 0.0f;
                if (own) {
                    g = s.q[n + lane];
                    for (int j = 0; j < m; ++j) g = fmaf(Quu[lane * ldd + j], xv[j], g);
                    gv[lane] = g;
                }
                const bool cl = own && ((x <= lo && g > 0.0f) || (x >= hi && g < 0.0f));
                held = (uint32_t)__ballot(cl);
                if (it > 0 && held == prev && full) { qp = 0; break; }   // a full Newton step on this very set: aug is current
                wsync();
                wave_for_2d(m, s.width, [&](int r, int j, int) {
                    const bool fr = !(held >> r & 1u);
                    float v;
                    if (j < m) v = (fr && !(held >> j & 1u)) ? Quu[r * ldd + j] : (r == j ? 1.0f : 0.0f);
                    else if (j == m) v = fr ? gv[r] : 0.0f;
                    else v = fr ? s.Q[(n + r) * ldd + (j - m - 1)] : 0.0f;
                    s.aug[r * lda + j] = v;
                });
                wsync();
                if (wave_gauss_jordan<false>(s.aug, lda, m, s.width, s.fac, s.prow)) { st |= TFMPC_ST_NOT_PD; qp = 0; break; }
                if (held == all_held) { qp = 0; break; }
                const float step = (own && !cl) ? -s.aug[lane * lda + m] : 0.0f;
                // Armijo backtracking along the projection arc; the decrease is g.d + 1/2 d^T Q_uu d (no cancellation)
                float alpha = 1.0f, xc = x;
                bool accepted = false;
                for (int bt = 0; bt < kQpBacktracks; ++bt) {
                    xc = fminf(fmaxf(fmaf(alpha, step, x), lo), hi);
                    const float dd = xc - x;
                    wsync();
                    if (own) dv[lane] = dd;
                    wsync();
                    float qd = 0.0f;
                    if (own)
                        for (int j = 0; j < m; ++j) qd = fmaf(Quu[lane * ldd + j], dv[j], qd);
                    const float gd = wave_sum(own ? g * dd : 0.0f);
                    const float df = gd + wave_sum(own ? 0.5f * dd * qd : 0.0f);
                    if (df < 0.0f && df <= kArmijo * gd) { accepted = true; break; }
                    alpha *= 0.5f;
                }
                if (!accepted) { qp = 0; break; }               // the rounding floor: x stays, aug belongs to `held`
                full = alpha == 1.0f && __ballot(own && xc != x + step) == 0;
                x = xc;
                prev = held;
                wsync();
                if (own) xv[lane] = x;
                wsync();
            }
            st |= qp;
            if (st & TFMPC_ST_NOT_PD) return st;

            // gains: rows of held controls exactly 0, K_f = -Q_uu,ff^-1 Q_ux,f ; k = x
            wave_for_2d(m, n, [&](int r, int j, int idx) {
                const float v = (held >> r & 1u) ? 0.0f : -s.aug[r * lda + m + 1 + j];
                s.K[r * ldn + j] = v;
                Kg[(size_t)t * m * n + idx] = v;
            });
            if (own) {
                kg[(size_t)t * m + lane] = x;
                kpart = fmaxf(kpart, fabsf(x));
            }
            if (maskg && lane == 0) maskg[t] = held;
            wsync();
            // V' = Q_xx + Q_xu K ; v' = q_x + Q_xu k (Schur forms: K_c = 0 and (Q_uu k + q_u)_f = 0 at the QP's optimum)
            wave_matmul_mfma(n, n, m,
                             [&](int i, int k) { return s.Q[i * ldd + n + k]; },
                             [&](int k, int j) { return s.K[k * ldn + j]; },
                             [&](int i, int j) { return s.Q[i * ldd + j]; },
                             [&](int i, int j, float v) { s.Vn[i * ldv + j] = v; });
            for (int i = lane; i < n; i += kWave) {
                float s1 = 0.0f;
                for (int k = 0; k < m; ++k) s1 = fmaf(s.Q[i * ldd + n + k], xv[k], s1);
                s.vn[i] = s.q[i] + s1;
            }
            float part = 0.0f;
            if (own) {
                float quk = 0.0f;
                for (int k = 0; k < m; ++k) quk = fmaf(Quu[lane * ldd + k], xv[k], quk);
                part = x * (0.5f * quk + s.q[n + lane]);
            }
            dV += wave_sum(part);
            wsync();
            wave_for_2d(n, n, [&](int i, int j, int) { s.V[i * ldn + j] = 0.5f * (s.Vn[i * ldv + j] + s.Vn[j * ldv + i]); });
            for (int i = lane; i < n; i += kWave) s.v[i] = s.vn[i];
            wsync();
        }
        // (|k| may be NaN only with a NaN dV, which the caller tests; fmaxf drops it here)
        kmax = wave_max(kpart);
        umax = wave_max(upart);
        return st;
    };

    // The candidate becomes the nominal.
    auto adopt = [&]() {
        wsync();                                                // the candidate is visible to every lane
        for (size_t i = lane; i < nx; i += kWave) xs[i] = cx[i];
        for (size_t i = lane; i < nu; i += kWave) us[i] = cu[i];
        for (size_t i = lane; i < nc; i += kWave) cs[i] = cc[i];
        wsync();
    };

    const int max_iter = p.max_iter > 0 ? p.max_iter : kDefaultPasses;
    const float tol = p.tol > 0.0f ? p.tol : kDefaultTol;
    int status = 0, reason = kReasonConverged, sweeps = 0, trusted = 0;

    float J = rollout(0.0f, true, xs, us, cs);
    wsync();                                                    // the nominal is visible to every lane
    if (!(J == J)) status |= TFMPC_ST_NAN;
    if (any_free && !status) {
        reason = kReasonPassCap;
        for (int pass = 0; pass < max_iter; ++pass) {
            float kmax, umax, dV;
            status = sweep(kmax, umax, dV);                     // the last sweep's bits: an earlier pass's are dropped
            ++sweeps;
            if (!(dV == dV)) status |= TFMPC_ST_NAN;
            if (status & (TFMPC_ST_NOT_PD | TFMPC_ST_NAN)) { reason = kReasonFailed; break; }
            wsync();                                            // the gains are visible to every lane
            if (kmax <= tol * fmaxf(1.0f, umax)) {
                // converged: the step is below tol but not below fp32 rounding, so it is applied in full, untested
                reason = kReasonConverged;
                if (kmax > 0.0f) {
                    J = rollout(1.0f, false, cx, cu, cc);
                    adopt();
                    if (!(J == J)) { status |= TFMPC_ST_NAN; reason = kReasonFailed; }
                }
                break;
            }
            // a predicted decrease below the rounding of J: J cannot rank candidates, the full step is taken untested
            const bool trust = -dV <= kTrustRatio * fmaxf(1.0f, fabsf(J)) && trusted < kTrustedInARow;
            trusted = trust ? trusted + 1 : 0;
            float alpha = 1.0f, Jn = J;
            bool accepted = false;
            for (int ls = 0; ls < kAlphas; ++ls) {
                Jn = rollout(alpha, false, cx, cu, cc);
                if (trust || Jn < J) { accepted = true; break; }
                alpha *= 0.5f;
            }
            if (!accepted) { reason = kReasonNoDecrease; break; }
            adopt();
            J = Jn;
            if (!(J == J)) { status |= TFMPC_ST_NAN; reason = kReasonFailed; break; }
        }
        if (reason == kReasonPassCap) status |= TFMPC_ST_MAX_ATTEMPTS;
    } else if (status) {
        reason = kReasonFailed;
    }

    if (status & (TFMPC_ST_NOT_PD | TFMPC_ST_NAN)) {
        const float qnan = __builtin_nanf("");
        for (size_t i = lane; i < nx; i += kWave) xs[i] = qnan;
        for (size_t i = lane; i < nu; i += kWave) us[i] = qnan;
        for (size_t i = lane; i < nc; i += kWave) cs[i] = qnan;
    }
    if (lane == 0) {
        p.iterations[b] = sweeps;
        a.status[b] = status;
        if (p.reason) p.reason[b] = reason;
    }
}

bool box_supported(int n, int m) { return m <= 32 && tv_smem_elems<false>(n, m) * sizeof(float) <= kMaxLdsBytes; }

size_t box_workspace_floats(int B, int n, int m, int T)
{
    return (size_t)B * ((size_t)T * m * (n + 1) + ((size_t)T + 1) * n + (size_t)T * m + ((size_t)T + 1));
}

}  // namespace

}  // namespace tfmpc

using namespace tfmpc;

extern "C" {

size_t tfmpc_tvlqr_box_solve_workspace_bytes(int B, int n, int m, int T)
{
    if (B <= 0 || n <= 0 || m <= 0 || T <= 0) return 0;
    return box_workspace_floats(B, n, m, T) * sizeof(float);
}

const char *tfmpc_tvlqr_box_solve_kernel_name(int n, int m, int T)
{
    (void)T;
    if (n <= 0 || m <= 0) return "invalid";
    return box_supported(n, m) ? "tv_box_wave" : "unsupported";
}

int tfmpc_tvlqr_box_solve_f32(int B, int n, int m, int T, const float *F, long sF_b, long sF_t, const float *f, long sf_b,
                              long sf_t, const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t,
                              const float *Cfin, long sCfin_b, const float *cfin, long scfin_b, const float *low, long slow_b,
                              long slow_t, const float *high, long shigh_b, long shigh_t, const float *x0, const float *u_init,
                              long su_b, int max_iter, float tol, float *states, float *actions, float *costs,
                              int32_t *iterations, int32_t *status, int32_t *reason, uint32_t *clamp_mask, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    if (B < 0 || n <= 0 || m <= 0 || T <= 0 || max_iter < 0 || !(tol >= 0.0f)) return TFMPC_ERR_ARG;
    if (!box_supported(n, m)) return TFMPC_ERR_UNSUPPORTED;
    if (B == 0) return TFMPC_OK;                                    // no-op: nothing is read
    if (!F || !f || !C || !c || !low || !high || !x0) return TFMPC_ERR_ARG;
    if (!Cfin != !cfin) return TFMPC_ERR_ARG;                       // both or neither
    for (long s : {sF_b, sF_t, sf_b, sf_t, sC_b, sC_t, sc_b, sc_t, sCfin_b, scfin_b, slow_b, slow_t, shigh_b, shigh_t, su_b})
        if (s < 0) return TFMPC_ERR_ARG;
    if (!states || !actions || !costs || !iterations || !status) return TFMPC_ERR_ARG;
    if (!workspace || workspace_bytes < tfmpc_tvlqr_box_solve_workspace_bytes(B, n, m, T)) return TFMPC_ERR_WORKSPACE;

    TvBoxArgs p{};
    TvLqrArgs &a = p.a;
    a.B = B; a.n = n; a.m = m; a.T = T;
    a.F = F; a.sF_b = sF_b; a.sF_t = sF_t;
    a.f = f; a.sf_b = sf_b; a.sf_t = sf_t;
    a.C = C; a.sC_b = sC_b; a.sC_t = sC_t;
    a.c = c; a.sc_b = sc_b; a.sc_t = sc_t;
    a.Cfin = Cfin; a.sCfin_b = sCfin_b;
    a.cfin = cfin; a.scfin_b = scfin_b;
    a.x0 = x0;
    float *w = static_cast<float *>(workspace);
    a.K = w; a.sK = (long)T * m * n; w += (size_t)B * T * m * n;
    a.k = w; a.sk = (long)T * m; w += (size_t)B * T * m;
    p.cx = w; w += (size_t)B * ((size_t)T + 1) * n;
    p.cu = w; w += (size_t)B * T * m;
    p.cc = w;
    a.states = states; a.actions = actions; a.costs = costs; a.status = status;
    p.low = low; p.slow_b = slow_b; p.slow_t = slow_t;
    p.high = high; p.shigh_b = shigh_b; p.shigh_t = shigh_t;
    p.u_init = u_init; p.su_b = su_b;
    p.max_iter = max_iter; p.tol = tol;
    p.iterations = iterations; p.reason = reason; p.clamp_mask = clamp_mask;

    const size_t smem = tv_smem_elems<false>(n, m) * sizeof(float);
    if (smem > 64 * 1024) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(tvlqr_box_solve_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
            return TFMPC_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(tvlqr_box_solve_kernel, dim3(B), dim3(kWave), smem, static_cast<hipStream_t>(stream), p);
    return hipGetLastError() == hipSuccess ? TFMPC_OK : TFMPC_ERR_LAUNCH;
}

}  // extern "C"
