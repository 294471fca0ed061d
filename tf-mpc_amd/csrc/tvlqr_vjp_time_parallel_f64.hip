// tvlqr_vjp_time_parallel_f64.hip -- gradients of the TIME-PARALLEL double-precision time-varying LQR
// (tfmpc_tvlqr_vjp_time_parallel_f64, include/tfmpc_hip.h): tfmpc_tvlqr_vjp_f64's contract with the
// adjoint solve replaced by a SEGMENTED ADJOINT that reuses the forward's gains and value function; n <= 32, m <= 32.
//
// The adjoint problem has the forward's F, C, C_fin and other linear terms (c~_t = g_t, c~_fin = g_T, f~ = 0, x~0 = 0), so
// it has the forward's K_t and V_t (V_T = C_fin); only its vector part is new.  With L_t = [I; K_t], A_t = F_t[:, :n],
// B_t = F_t[:, n:] and the closed-loop transition Phi_t = F_t L_t = A_t + B_t K_t:
//   backward  v~_T = g_T,  v~_t = a_t + Phi_t^T v~_{t+1},          a_t = L_t^T g_t = g_t[:n] + K_t^T g_t[n:]
//   per step  Q_uu,t = C_t[n:, n:] + B_t^T V_{t+1} B_t,  k~_t = -(r_t + E_t v~_{t+1}),  [r_t | E_t] = Q_uu,t^-1 [g_t[n:] | B_t^T]
//   forward   dx_0 = 0,  du_t = K_t dx_t + k~_t,  dx_{t+1} = Phi_t dx_t + w_t,          w_t = B_t k~_t
// Both recursions are affine in the closed-loop Phi_t, so a segment [s, e) condenses to ONE matrix
// M = Phi_{e-1} ... Phi_s and one offset per direction: v~_s = M^T v~_e + beta, dx_e = M dx_s + gamma.  There is no Riccati
// step and no n-sized elimination anywhere; the only elimination is the pivot-free m x m Q_uu, once per (b, t), off the
// serial path.  Launches on the caller's stream (no allocation, no sync, no atomics):
//   1. the fold                 tvlqr_vjp_f64.hip's (g_t, g_T, the default final cost's copy)
//   2. tp_vjp_step_kernel       one wave per (b, t): Phi_t, a_t, r_t, E_t^T; a non-positive pivot: TFMPC_ST_NOT_PD
//   3. tp_vjp_condense_kernel   one wave per (b, segment): M on the f64 matrix cores, beta
//   4. tp_vjp_stitch_back       one wave per instance: the status (OR over the steps), v~ at every segment's end
//   5. tp_vjp_expand_back       one wave per (b, segment): v~_t, k~_t, w_t of its steps, then gamma
//   6. tp_vjp_stitch_fwd        one wave per instance: dx at every segment's start
//   7. tp_vjp_expand_fwd        one wave per (b, segment): dx_t, du_t of its steps; the last segment writes dx_T
//   8. costates and batch sums  tvlqr_vjp_f64.hip's, unchanged, on the forward's V and the v~, dx, du of 5 and 7
// A wave touches its own instance only and every sum has a fixed order: an instance's bits depend on neither B nor its
// position, and repeated calls give identical bits.  The build is -ffp-contract=off: every fused multiply-add is a
// written fma().  No scratch memory.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lqr_kernels.h"
#include "options.h"
#include "tvlqr_kernels.h"
#include "tvlqr_vjp_common.h"
#include "wave_ops_f64.h"

using namespace tfmpc;

namespace {

struct TpVjpArgs {
    int B, n, m, T, segments, len;
    const double *F, *C;
    long sF_b, sF_t, sC_b, sC_t;
    const double *Cf;                // V_T: the final cost, explicit or the fold's copy of the default
    long sCf_b;
    const double *K, *V;             // the forward's K[B][T][m][n], V[B][T][n][n]
    const double *g, *gT;            // the fold's g_t [B][T][d], g_T [B][n]
    double *Phi, *av, *r, *Et, *w;   // per (b, t): Phi_t [n][n], a_t [n], r_t [m], E_t^T [n][m], w_t [n]
    double *vt;                      // v~_t [B][T][n]
    double *dS, *dA;                 // dx [B][T + 1][n]; du [B][T][m] (k~_t between 5 and 7)
    double *M, *beta, *gamma;        // per (b, segment): [n][n], [n], [n]
    double *vend, *xstart;           // per (b, segment): v~ at its end, dx at its start
    int32_t *st_step;                // [B][T]
    int32_t *status;                 // [B]
};

__device__ __forceinline__ int seg_end(const TpVjpArgs &a, int t0) { return a.T - t0 < a.len ? a.T : t0 + a.len; }

// LDS of a step wave, in doubles: F_t, K_t, V_{t+1}, V_{t+1} B_t, the augmented block m x (m + 1 + n), multipliers, g_t
__host__ __device__ constexpr size_t step_smem_elems(int n, int m)
{
    return (size_t)n * odd_ld(n + m) + (size_t)m * odd_ld(n) + (size_t)n * odd_ld(n) + (size_t)n * odd_ld(m) +
           (size_t)m * odd_ld(m + 1 + n) + m + n + m;
}

// ---- 2. per step ---------------------------------------------------------------------------------------------------------
template <int MAXD>
__global__ __launch_bounds__(kWave) void tp_vjp_step_kernel(TpVjpArgs a)
{
    extern __shared__ double smem_tpv[];
    const int n = a.n, m = a.m, T = a.T, d = n + m, lane = lane_id();
    const size_t bt = blockIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)T), t = (int)blockIdx.x - b * T;
    const int ldd = odd_ld(d), ldn = odd_ld(n), ldm = odd_ld(m), wR = m + 1 + n, ldR = odd_ld(wR);
    double *p = smem_tpv;
    double *F = p; p += n * ldd;
    double *Kt = p; p += m * ldn;
    double *Vn = p; p += n * ldn;
    double *W = p; p += n * ldm;
    double *aug = p; p += m * ldR;
    double *fac = p; p += m;
    double *g = p;

    load_matrix(F, ldd, tv_at(a.F, a.sF_b, a.sF_t, b, t), n, d);
    load_matrix(Kt, ldn, a.K + bt * m * n, m, n);
    load_matrix(Vn, ldn, t == T - 1 ? a.Cf + (size_t)b * a.sCf_b : a.V + (bt + 1) * n * n, n, n);
    for (int i = lane; i < d; i += kWave) g[i] = a.g[bt * d + i];
    wsync();
    // Phi_t = A_t + B_t K_t ; W = V_{t+1} B_t ; a_t = g_x + K_t^T g_u
    double *Phi = a.Phi + bt * n * n;
    wave_matmul_f64<MAXD>(n, n, m, [&](int i, int k) { return F[i * ldd + n + k]; }, [&](int k, int j) { return Kt[k * ldn + j]; },
                          [&](int i, int j) { return F[i * ldd + j]; }, [&](int i, int j, double x) { Phi[i * n + j] = x; });
    wave_matmul_f64<MAXD>(n, m, n, [&](int i, int k) { return Vn[i * ldn + k]; }, [&](int k, int j) { return F[k * ldd + n + j]; },
                          [](int, int) { return 0.0; }, [&](int i, int j, double x) { W[i * ldm + j] = x; });
    for (int i = lane; i < n; i += kWave) {
        double s = 0.0;
        for (int k = 0; k < m; ++k) s = fma(Kt[k * ldn + i], g[n + k], s);
        a.av[bt * n + i] = g[i] + s;
    }
    wsync();
    // [Q_uu | g_u | B_t^T] -> [I | r_t | E_t], without pivoting
    const double *Ct = tv_at(a.C, a.sC_b, a.sC_t, b, t);
    wave_matmul_f64<MAXD>(m, m, n, [&](int i, int k) { return F[k * ldd + n + i]; }, [&](int k, int j) { return W[k * ldm + j]; },
                          [&](int i, int j) { return Ct[(size_t)(n + i) * d + n + j]; },
                          [&](int i, int j, double x) { aug[i * ldR + j] = x; });
    wave_for_2d(m, n + 1, [&](int i, int j, int) { aug[i * ldR + m + j] = j == 0 ? g[n + i] : F[(j - 1) * ldd + n + i]; });
    wsync();
    const int bad = wave_gauss_jordan<false>(aug, ldR, m, wR, fac, (double *)nullptr);
    for (int i = lane; i < m; i += kWave) a.r[bt * m + i] = aug[i * ldR + m];
    double *Et = a.Et + bt * n * m;
    wave_for_2d(n, m, [&](int j, int i, int idx) { Et[idx] = aug[i * ldR + m + 1 + j]; });
    if (lane == 0) a.st_step[bt] = bad ? TFMPC_ST_NOT_PD : 0;
}

// ---- 3. condense: M = Phi_{e-1} ... Phi_s, beta = a_s + Phi_s^T (a_{s+1} + ... + Phi_{e-2}^T a_{e-1}) --------------------------
__host__ __device__ constexpr size_t condense_smem_elems(int n) { return (size_t)3 * n * odd_ld(n) + 2 * n; }

template <int MAXD>
__global__ __launch_bounds__(kWave) void tp_vjp_condense_kernel(TpVjpArgs a)
{
    extern __shared__ double smem_tpv[];
    const int n = a.n, T = a.T, lane = lane_id(), ldn = odd_ld(n);
    const size_t w = blockIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)a.segments), seg = (int)blockIdx.x - b * a.segments;
    const int t0 = seg * a.len, t1 = seg_end(a, t0);
    double *p = smem_tpv;
    double *Mc = p; p += n * ldn;                            // the product so far
    double *Mn = p; p += n * ldn;
    double *Ph = p; p += n * ldn;
    double *bc = p; p += n;
    double *bn = p;
    for (int t = t1 - 1; t >= t0; --t) {
        const size_t bt = (size_t)b * T + t;
        const bool first = t == t1 - 1;
        load_matrix(first ? Mc : Ph, ldn, a.Phi + bt * n * n, n, n);
        const double *at = a.av + bt * n;
        if (first) {
            for (int i = lane; i < n; i += kWave) bc[i] = at[i];
            lds_sync();
            continue;
        }
        lds_sync();
        wave_matmul_f64<MAXD>(n, n, n, [&](int i, int k) { return Mc[i * ldn + k]; }, [&](int k, int j) { return Ph[k * ldn + j]; },
                              [](int, int) { return 0.0; }, [&](int i, int j, double x) { Mn[i * ldn + j] = x; });
        for (int i = lane; i < n; i += kWave) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s = fma(Ph[k * ldn + i], bc[k], s);
            bn[i] = at[i] + s;
        }
        lds_sync();
        double *x;
        x = Mc; Mc = Mn; Mn = x;
        x = bc; bc = bn; bn = x;
    }
    store_matrix(a.M + w * n * n, Mc, ldn, n, n);
    for (int i = lane; i < n; i += kWave) a.beta[w * n + i] = bc[i];
}

// ---- 4. the status, and v~ at every segment's end: v~_start = M^T v~_end + beta -------------------------------------------
__global__ __launch_bounds__(kWave) void tp_vjp_stitch_back_kernel(TpVjpArgs a)
{
    __shared__ double vb[2][32];
    const int n = a.n, T = a.T, P = a.segments, lane = lane_id();
    const int b = blockIdx.x;
    const size_t w0 = (size_t)b * P;
    int mine = 0;
    for (int t = lane; t < T; t += kWave) mine |= a.st_step[(size_t)b * T + t];
    int status = 0;
    for (int bit = 0; bit < 8; ++bit)
        if (__ballot(mine >> bit & 1)) status |= 1 << bit;
    if (lane == 0) a.status[b] = status;
    double *vc = vb[0], *vn = vb[1];
    if (lane < n) vc[lane] = a.gT[(size_t)b * n + lane];
    lds_sync();
    for (int s = P - 1; s >= 0; --s) {
        if (lane < n) a.vend[(w0 + s) * n + lane] = vc[lane];
        if (s == 0) break;
        if (lane < n) {
            const double *Mg = a.M + (w0 + s) * n * n;
            double sum = 0.0;
            for (int k = 0; k < n; ++k) sum = fma(Mg[k * n + lane], vc[k], sum);
            vn[lane] = a.beta[(w0 + s) * n + lane] + sum;
        }
        lds_sync();
        double *x = vc; vc = vn; vn = x;
    }
}

// ---- 5. v~_t, k~_t, w_t of a segment's steps, then gamma = w_{e-1} + Phi_{e-1} (w_{e-2} + ... + Phi_{s+1} w_s) ---------------
__global__ __launch_bounds__(kWave) void tp_vjp_expand_back_kernel(TpVjpArgs a)
{
    __shared__ double vb[2][32], kt[32];
    const int n = a.n, m = a.m, T = a.T, d = n + m, lane = lane_id();
    const size_t w = blockIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)a.segments), seg = (int)blockIdx.x - b * a.segments;
    const int t0 = seg * a.len, t1 = seg_end(a, t0);
    double *vc = vb[0], *vn = vb[1];
    if (lane < n) vc[lane] = a.vend[w * n + lane];
    lds_sync();
    for (int t = t1 - 1; t >= t0; --t) {
        const size_t bt = (size_t)b * T + t;
        if (lane < m) {              // k~_t = -(r_t + E_t v~_{t+1})
            const double *Et = a.Et + bt * n * m;
            double s = a.r[bt * m + lane];
            for (int k = 0; k < n; ++k) s = fma(Et[k * m + lane], vc[k], s);
            kt[lane] = -s;
            a.dA[bt * m + lane] = -s;
        }
        if (lane < n) {              // v~_t = a_t + Phi_t^T v~_{t+1}
            const double *Phi = a.Phi + bt * n * n;
            double s = 0.0;
            for (int k = 0; k < n; ++k) s = fma(Phi[k * n + lane], vc[k], s);
            s = a.av[bt * n + lane] + s;
            vn[lane] = s;
            a.vt[bt * n + lane] = s;
        }
        lds_sync();
        if (lane < n) {              // w_t = B_t k~_t
            const double *Fi = tv_at(a.F, a.sF_b, a.sF_t, b, t) + (size_t)lane * d + n;
            double s = 0.0;
            for (int k = 0; k < m; ++k) s = fma(Fi[k], kt[k], s);
            a.w[bt * n + lane] = s;
        }
        lds_sync();                  // kt is rewritten by the next step
        double *x = vc; vc = vn; vn = x;
    }
    // forwards over the same steps (lane i reads back the w_t[i] it stored itself)
    if (lane < n) vc[lane] = 0.0;
    lds_sync();
    for (int t = t0; t < t1; ++t) {
        const size_t bt = (size_t)b * T + t;
        if (lane < n) {
            const double *Pi = a.Phi + bt * n * n + (size_t)lane * n;
            double s = 0.0;
            for (int k = 0; k < n; ++k) s = fma(Pi[k], vc[k], s);
            vn[lane] = a.w[bt * n + lane] + s;
        }
        lds_sync();
        double *x = vc; vc = vn; vn = x;
    }
    if (lane < n) a.gamma[w * n + lane] = vc[lane];
}

// ---- 6. dx at every segment's start: dx_end = M dx_start + gamma ---------------------------------------------------------
__global__ __launch_bounds__(kWave) void tp_vjp_stitch_fwd_kernel(TpVjpArgs a)
{
    __shared__ double xb[2][32];
    const int n = a.n, P = a.segments, lane = lane_id();
    const size_t w0 = (size_t)blockIdx.x * P;
    double *xc = xb[0], *xn = xb[1];
    if (lane < n) xc[lane] = 0.0;
    lds_sync();
    for (int s = 0; s < P; ++s) {
        if (lane < n) a.xstart[(w0 + s) * n + lane] = xc[lane];
        if (s == P - 1) break;
        if (lane < n) {
            const double *Mi = a.M + (w0 + s) * n * n + (size_t)lane * n;
            double sum = 0.0;
            for (int k = 0; k < n; ++k) sum = fma(Mi[k], xc[k], sum);
            xn[lane] = a.gamma[(w0 + s) * n + lane] + sum;
        }
        lds_sync();
        double *x = xc; xc = xn; xn = x;
    }
}

// ---- 7. dx_t, du_t = K_t dx_t + k~_t of a segment's steps; dx_{t+1} = Phi_t dx_t + w_t -----------------------------------
__global__ __launch_bounds__(kWave) void tp_vjp_expand_fwd_kernel(TpVjpArgs a)
{
    __shared__ double xb[2][32];
    const int n = a.n, m = a.m, T = a.T, lane = lane_id();
    const size_t w = blockIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)a.segments), seg = (int)blockIdx.x - b * a.segments;
    const int t0 = seg * a.len, t1 = seg_end(a, t0);
    double *xc = xb[0], *xn = xb[1];
    if (lane < n) xc[lane] = a.xstart[w * n + lane];
    lds_sync();
    for (int t = t0; t < t1; ++t) {
        const size_t bt = (size_t)b * T + t;
        if (lane < n) {
            a.dS[((size_t)b * (T + 1) + t) * n + lane] = xc[lane];
            const double *Pi = a.Phi + bt * n * n + (size_t)lane * n;
            double s = 0.0;
            for (int k = 0; k < n; ++k) s = fma(Pi[k], xc[k], s);
            xn[lane] = a.w[bt * n + lane] + s;
        }
        if (lane < m) {
            const double *Ki = a.K + bt * m * n + (size_t)lane * n;
            double s = 0.0;
            for (int k = 0; k < n; ++k) s = fma(Ki[k], xc[k], s);
            a.dA[bt * m + lane] = a.dA[bt * m + lane] + s;
        }
        lds_sync();
        double *x = xc; xc = xn; xn = x;
    }
    if (t1 == T && lane < n) a.dS[((size_t)b * (T + 1) + T) * n + lane] = xc[lane];
}

// ---- workspace, in doubles, every array rounded up to 64 ------------------------------------------------------------------
struct SegmentTable { int len, count; };

// DESIGN.md 3.19's table: `segments` clamped to T, len = ceil(T / segments), count = ceil(T / len)
SegmentTable segment_table(int T, int segments)
{
    if (segments > T) segments = T;
    const long len = ((long)T + segments - 1) / segments;
    return {(int)len, (int)((T + len - 1) / len)};
}

struct Layout : VjpPrefix {
    size_t Phi, av, r, Et, w, vt, P, partial, M, beta, gamma, vend, xstart, st, total;
};

Layout layout(int B, int n, int m, int T, int count)
{
    Layout L{};
    const size_t BT = (size_t)B * T, BP = (size_t)B * count;
    size_t o = vjp_prefix(L, B, n, m, T);
    L.Phi = o; o += up64(BT * n * n);
    L.av = o; o += up64(BT * n);
    L.r = o; o += up64(BT * m);
    L.Et = o; o += up64(BT * n * m);
    L.w = o; o += up64(BT * n);
    L.vt = o; o += up64(BT * n);
    L.P = o; o += up64(BT * 2 * n);
    L.partial = o; o += vjp_partial_elems(B, n, m, T);
    L.M = o; o += up64(BP * n * n);
    L.beta = o; o += up64(BP * n);
    L.gamma = o; o += up64(BP * n);
    L.vend = o; o += up64(BP * n);
    L.xstart = o; o += up64(BP * n);
    L.st = o; o += up64((BT + 1) / 2);                       // 32-bit words
    L.total = o;
    return L;
}

template <class K>
int launch_waves(K kern, size_t blocks, size_t smem, hipStream_t stream, const TpVjpArgs &a)
{
    return launch_with_lds(kern, (unsigned)blocks, kWave, smem, stream, a);
}

}  // namespace

extern "C" {

size_t tfmpc_tvlqr_vjp_time_parallel_workspace_bytes_f64(int B, int n, int m, int T, int segments)
{
    if (B <= 0 || n <= 0 || m <= 0 || T <= 0 || segments < 1) return 0;
    const SegmentTable tab = segment_table(T, segments);
    if (tab.count == 1) return tfmpc_tvlqr_vjp_workspace_bytes_f64(B, n, m, T);
    return layout(B, n, m, T, tab.count).total * sizeof(double);
}

int tfmpc_tvlqr_vjp_time_parallel_f64(int B, int n, int m, int T, const double *F, long sF_b, long sF_t, const double *f,
                                      long sf_b, long sf_t, const double *C, long sC_b, long sC_t, const double *c, long sc_b,
                                      long sc_t, const double *Cfin, long sCfin_b, const double *cfin, long scfin_b,
                                      const double *states, const double *actions, const double *v, const double *K,
                                      const double *V, const double *g_states, const double *g_actions, const double *g_costs,
                                      double *dF, long sdF_b, long sdF_t, double *df, long sdf_b, long sdf_t, double *dC,
                                      long sdC_b, long sdC_t, double *dc, long sdc_b, long sdc_t, double *dCfin, long sdCfin_b,
                                      double *dcfin, long sdcfin_b, double *dx0, long sdx0_b, int32_t *status, int segments,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    if (B < 0 || n <= 0 || m <= 0 || T <= 0) return TFMPC_ERR_ARG;
    if (!tvlqr_f64_supported(n, m)) return TFMPC_ERR_UNSUPPORTED;
    if (segments < 1) return TFMPC_ERR_ARG;
    if (B == 0) return TFMPC_OK;
    if (!v) return TFMPC_ERR_ARG;
    const SegmentTable tab = segment_table(T, segments);
    if (tab.count == 1)              // one segment is the sequential adjoint: its checks, its workspace rule, its bits
        return tfmpc_tvlqr_vjp_f64(B, n, m, T, F, sF_b, sF_t, f, sf_b, sf_t, C, sC_b, sC_t, c, sc_b, sc_t, Cfin, sCfin_b, cfin,
                                   scfin_b, states, actions, v, g_states, g_actions, g_costs, dF, sdF_b, sdF_t, df, sdf_b, sdf_t,
                                   dC, sdC_b, sdC_t, dc, sdc_b, sdc_t, dCfin, sdCfin_b, dcfin, sdcfin_b, dx0, sdx0_b, status,
                                   workspace, workspace_bytes, stream);
    if (!K || !V) return TFMPC_ERR_ARG;
    const VjpCall<double> call{B, n, m, T, F, sF_b, sF_t, f, sf_b, sf_t, C, sC_b, sC_t, c, sc_b, sc_t, Cfin, sCfin_b, cfin, scfin_b,
                               states, actions, g_states, g_actions, g_costs, dF, sdF_b, sdF_t, df, sdf_b, sdf_t, dC, sdC_b, sdC_t,
                               dc, sdc_b, sdc_t, dCfin, sdCfin_b, dcfin, sdcfin_b, dx0, sdx0_b, status, workspace, workspace_bytes,
                               stream};
    if (const int rc = vjp_check_call<double>(call, nullptr, true); rc != TFMPC_OK) return rc;
    const Layout L = layout(B, n, m, T, tab.count);
    if (!workspace || workspace_bytes < L.total * sizeof(double)) return TFMPC_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) % sizeof(double)) return TFMPC_ERR_ARG;      // doubles are carved from it
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *w = static_cast<double *>(workspace);

    VjpBase<double> base{};          // the final cost's place and stride, the fold's arrays
    vjp_fill_base<double>(base, call, w, L);
    TpVjpArgs a{};
    a.B = B; a.n = n; a.m = m; a.T = T; a.segments = tab.count; a.len = tab.len;
    a.F = F; a.sF_b = sF_b; a.sF_t = sF_t;
    a.C = C; a.sC_b = sC_b; a.sC_t = sC_t;
    a.Cf = base.Cf; a.sCf_b = base.sCf_b;
    a.K = K; a.V = V;
    a.g = w + L.ct; a.gT = w + L.cT;
    a.Phi = w + L.Phi; a.av = w + L.av; a.r = w + L.r; a.Et = w + L.Et; a.w = w + L.w;
    a.vt = w + L.vt; a.dS = w + L.dS; a.dA = w + L.dA;
    a.M = w + L.M; a.beta = w + L.beta; a.gamma = w + L.gamma; a.vend = w + L.vend; a.xstart = w + L.xstart;
    a.st_step = reinterpret_cast<int32_t *>(w + L.st);
    a.status = status;

    // TFMPC_TVLQR_TP_PHASES = 1 .. 6: stop after the fold and the step kernel / the condense / ... / the forward expand
    // -- for the phase split of tools/tvlqr_time_parallel_grad_rate.py only; no output is written, and the call says so
    const int phases = option_int(kOptTvlqrTpPhases, 7);
    const bool small = wave16(n, m);
    const size_t BT = (size_t)B * T, BP = (size_t)B * tab.count;
    int rc;
    if ((rc = tvlqr_vjp_f64_fold_launch(call, w, L)) != TFMPC_OK) return rc;
    const size_t step_smem = step_smem_elems(n, m) * sizeof(double);
    rc = small ? launch_waves(tp_vjp_step_kernel<16>, BT, step_smem, s, a) : launch_waves(tp_vjp_step_kernel<32>, BT, step_smem, s, a);
    if (rc != TFMPC_OK) return rc;
    if (phases == 1) return TFMPC_TVLQR_TP_STOPPED;
    const size_t cond_smem = condense_smem_elems(n) * sizeof(double);
    rc = small ? launch_waves(tp_vjp_condense_kernel<16>, BP, cond_smem, s, a)
               : launch_waves(tp_vjp_condense_kernel<32>, BP, cond_smem, s, a);
    if (rc != TFMPC_OK) return rc;
    if (phases == 2) return TFMPC_TVLQR_TP_STOPPED;
    if ((rc = launch_waves(tp_vjp_stitch_back_kernel, B, 0, s, a)) != TFMPC_OK) return rc;
    if (phases == 3) return TFMPC_TVLQR_TP_STOPPED;
    if ((rc = launch_waves(tp_vjp_expand_back_kernel, BP, 0, s, a)) != TFMPC_OK) return rc;
    if (phases == 4) return TFMPC_TVLQR_TP_STOPPED;
    if ((rc = launch_waves(tp_vjp_stitch_fwd_kernel, B, 0, s, a)) != TFMPC_OK) return rc;
    if (phases == 5) return TFMPC_TVLQR_TP_STOPPED;
    if ((rc = launch_waves(tp_vjp_expand_fwd_kernel, BP, 0, s, a)) != TFMPC_OK) return rc;
    if (phases == 6) return TFMPC_TVLQR_TP_STOPPED;
    return tvlqr_vjp_f64_costates_launch(call, w, L, v, V, w + L.vt, w + L.P, w + L.partial);
}

}  // extern "C"
