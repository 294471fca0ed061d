// tvlqr_box_vjp_f64.hip -- gradients of the DOUBLE-PRECISION control-limited time-varying LQR optimum
// (tfmpc_tvlqr_box_vjp_f64, include/tfmpc_hip.h).
//
// The contract is tfmpc_tvlqr_box_vjp_f32's (tvlqr_vjp.hip): a control whose bits equal low's or high's is
// held, du = 0 in the adjoint.  The costates are tvlqr_vjp_f64.hip's, the gradient of the value function
// on the optimal trajectory -- here of the REDUCED problem, held controls fixed at their bounds and free ones optimised:
//   lam_{t+1}  = V^m_{t+1} x_{t+1}  + v^m_{t+1}
//   dlam_{t+1} = V^m_{t+1} dx_{t+1} + v~_{t+1}
// V^m: the Riccati sequence of the masked model (it does not depend on linear terms: the adjoint solve produces it);
// v~: the masked adjoint solve's v; v^m: the v of the same masked model with the forward's reduced linear terms
// f^_t = f_t + F_t[:, n + H_t] u_{H_t}, c^_t = c_t + C_t[:, n + H_t] u_{H_t} and the true final cost.  Nothing the
// forward exports gives v^m, so a second masked backward sweep computes it.
// Launches on the caller's stream, no allocation, no sync, no atomics:
//   1. box_fold_f64_kernel     fold_body<double, true> (tvlqr_vjp_common.h: g_t, the held-set word, c~ with the held entries
//                              zeroed, the unmasked g_u), and f^_t, c^_t per (b, t).
//   2. the masked sweep        (tvlqr_solve_masked_f64) with c~ = g, f~ = 0, x~0 = 0, final cost (C_fin, g_T) -> dz, V^m, v~.
//   3. the masked sweep        backward only, with (f^, c^) and the true final cost -> v^m; then box_status_or_kernel: the
//                              status is the OR of both sweeps'.
//   4. box_costate_kernel      tvlqr_vjp_f64.hip's vjp_costate_kernel, one wavefront per (b, t) (<LOOP = true>: per instance,
//                              for per-instance outputs with time stride 0), in which lane i < m of a held control also forms
//                              r_t[n + i] = (C_t dz_t + g_t + F_t^T dlam_{t+1})[n + i], the gradient of the bound the control
//                              sits on (low when it equals both); free controls and the other bound get exact zeros.
//   5. the batch sums          vjp_shared_sums<double> for the model's gradients, box_reduce_bounds_f64 /
//                              box_reduce_final_f64 (tvlqr_vjp.hip's pair in double, the same fixed orders) for the bounds'.
// An instance with a status bit set contributes NaN (its own rows, dlow / dhigh included, and every batch sum that
// includes it).  The build is -ffp-contract=off: every fused multiply-add is a written fma().  No scratch memory.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "tvlqr_kernels.h"
#include "tvlqr_vjp_common.h"

using namespace tfmpc;

namespace {

using Out = OutT<double>;

struct VjpArgs : VjpBase<double> {
    const double *v;                 // v^m[B][T][n]: the forward-value sweep's
    const double *V, *vt;            // the adjoint sweep's V^m[B][T][n][n], v~[B][T][n] (v~_0: the base's a0)
};

struct BoxArgs : BoxArgsT<double> {
    const double *f;                 // the fold's second job: f^ [B][T][n], c^ [B][T][d]
    long sf_b, sf_t;
    double *fhat, *chat;
    double *gu;                      // [B][T][m]: the fold's unmasked g_u
};

// bits of the costate kernel's `want` beyond the model's kinds: dlow / dhigh written in place, or as a record per (b, t)
enum BoxKind { kLo = kKinds, kHi, kRecLo, kRecHi };
constexpr unsigned kBoxBits = 1u << kLo | 1u << kHi | 1u << kRecLo | 1u << kRecHi;

// ---- 1. fold ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWaveThreads) box_fold_f64_kernel(VjpArgs a, double *ct, double *cT, double *Cfe, double *zer,
                                                                    BoxArgs bx)
{
    {
        BoxArgsT<double> fb = bx;
        fb.Rlo = bx.gu;
        fold_body<double, true>(a, ct, cT, Cfe, zer, &fb);
    }
    const int n = a.n, m = a.m, T = a.T, d = n + m, L = threadIdx.x;
    const int b = (int)(blockIdx.x / (T + 1)), t = (int)(blockIdx.x % (T + 1));
    if (t == T) return;
    // f^_t = f_t + F_t[:, n + H] u_H, c^_t = c_t + C_t[:, n + H] u_H.  The held set is formed once more, by fold_body's
    // own test on the same bits: its word lives in fold_body (shared with the fp32 fold, whose text stays), and reading
    // back the copy lane 0 has just stored would need a fence; m loads and a ballot are cheaper.
    const double *u = a.actions + ((size_t)b * T + t) * m;
    bool on = false;
    if (L < m)
        on = same_bits(u[L], tv_at(bx.low, bx.slo_b, bx.slo_t, b, t)[L]) || same_bits(u[L], tv_at(bx.high, bx.shi_b, bx.shi_t, b, t)[L]);
    const uint32_t held = (uint32_t)__ballot(on);
    const double *Ft = tv_at(a.F, a.sF_b, a.sF_t, b, t), *Ct = tv_at(a.C, a.sC_b, a.sC_t, b, t);
    const double *ft = tv_at(bx.f, bx.sf_b, bx.sf_t, b, t), *cv = tv_at(a.c, a.sc_b, a.sc_t, b, t);
    for (int i = L; i < d; i += kWaveThreads) {
        double sc = cv[i], sf = i < n ? ft[i] : 0.0;
        for (uint32_t w = held; w; w &= w - 1) {
            const int j = __ffs((int)w) - 1;
            sc = fma(Ct[(size_t)i * d + n + j], u[j], sc);
            if (i < n) sf = fma(Ft[(size_t)i * d + n + j], u[j], sf);
        }
        bx.chat[((size_t)b * T + t) * d + i] = sc;
        if (i < n) bx.fhat[((size_t)b * T + t) * n + i] = sf;
    }
}

// ---- 3. the status of the call: both sweeps' ---------------------------------------------------------------------------
__global__ void box_status_or_kernel(int32_t *status, const int32_t *second, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) status[b] |= second[b];
}

// ---- 4. value-function costates, per-instance gradients, the bounds' gradients ---------------------------------------
__device__ inline void emit(const Out &o, int b, int t, bool first, int e, double v)
{
    double *p = o.p + (size_t)b * o.sb + (size_t)t * o.st + e;
    if (!first) v += *p;             // time-shared: accumulate in time order (this lane owns element e throughout)
    *p = v;
}

__host__ __device__ inline size_t costate_smem_elems(int n, int m)
{
    return (size_t)n * (n + 1) + 4 * (size_t)n + 2 * (size_t)(n + m);
}

// want: bit k = emit output k here.  LOOP = false: grid B T, block (b, t), every emitted output has its own slot per
// step (or T == 1).  LOOP = true: grid B, the block walks the steps backwards and accumulates in the output.
template <bool LOOP>
__global__ void __launch_bounds__(kWaveThreads) box_costate_kernel(VjpArgs a, unsigned want, bool store_factors, BoxArgs bx)
{
    extern __shared__ double sm[];
    const int n = a.n, m = a.m, T = a.T, d = n + m, L = threadIdx.x;
    const int b = LOOP ? (int)blockIdx.x : (int)(blockIdx.x / T);
    double *sV = sm, *x1 = sV + (size_t)n * (n + 1), *dx1 = x1 + n, *lam = dx1 + n, *dlam = lam + n, *z = dlam + n, *dz = z + d;
    const double poison = poison_of<double>(a.status, ~0, b);
    const Out &oF = a.o[kF], &of = a.o[kf], &oC = a.o[kC], &oc = a.o[kc];
    for (int t = LOOP ? T - 1 : (int)(blockIdx.x % T); t >= 0; --t) {
        const bool last = t == T - 1, first = last || !LOOP;
        // V_{t+1} [n][n + 1], x_{t+1}, dx_{t+1}, z_t, dz_t
        const double *Vn = last ? a.Cf + (size_t)b * a.sCf_b : a.V + ((size_t)b * T + t + 1) * n * n;
        for (int e = L; e < n * n; e += kWaveThreads) sV[(e / n) * (n + 1) + e % n] = Vn[e];
        const double *xs = a.states + ((size_t)b * (T + 1) + t) * n, *dxs = a.dS + ((size_t)b * (T + 1) + t) * n;
        const double *u = a.actions + ((size_t)b * T + t) * m, *du = a.dA + ((size_t)b * T + t) * m;
        for (int i = L; i < d; i += kWaveThreads) {
            z[i] = i < n ? xs[i] : u[i - n];
            dz[i] = (i < n ? dxs[i] : du[i - n]) + poison;
        }
        for (int i = L; i < n; i += kWaveThreads) {
            x1[i] = xs[n + i] + poison;
            dx1[i] = dxs[n + i] + poison;
        }
        const double gc = a.gc ? a.gc[(size_t)b * (T + 1) + t] : 0.0;
        const double gcT = a.gc ? a.gc[(size_t)b * (T + 1) + T] : 0.0;     // used at the last step only
        __syncthreads();
        // lam_{t+1} = V_{t+1} x_{t+1} + v_{t+1}, dlam_{t+1} = V_{t+1} dx_{t+1} + v~_{t+1}: lane r takes row r % n of one of them
        const double *fv = last ? a.cf + (size_t)b * a.scf_b : a.v + ((size_t)b * T + t + 1) * n;
        const double *av = last ? a.cT + (size_t)b * n : a.vt + ((size_t)b * T + t + 1) * n;
        for (int r = L; r < 2 * n; r += kWaveThreads) {
            const int i = r % n;
            const bool adj = r >= n;
            const double *rhs = adj ? dx1 : x1, *Vi = sV + (size_t)i * (n + 1);
            double s = (adj ? av : fv)[i];
            for (int j = 0; j < n; ++j) s = fma(Vi[j], rhs[j], s);
            (adj ? dlam : lam)[i] = s;
        }
        __syncthreads();
        if (want >> kF & 1u)
            for (int e = L; e < n * d; e += kWaveThreads) {
                const int i = e / d, j = e % d;
                emit(oF, b, t, first, e, fma(dlam[i], z[j], lam[i] * dz[j]));
            }
        if (want >> kf & 1u)
            for (int i = L; i < n; i += kWaveThreads) emit(of, b, t, first, i, dlam[i]);
        if (want >> kC & 1u)
            for (int e = L; e < d * d; e += kWaveThreads) {
                const int i = e / d, j = e % d;
                double v = 0.5 * (dz[i] * z[j] + z[i] * dz[j] + gc * z[i] * z[j]);
                if (a.dflt && last && i < n && j < n) v += 0.5 * (dx1[i] * x1[j] + x1[i] * dx1[j] + gcT * x1[i] * x1[j]);
                emit(oC, b, t, first, e, v);
            }
        if (want >> kc & 1u)
            for (int i = L; i < d; i += kWaveThreads) {
                double v = dz[i] + gc * z[i];
                if (a.dflt && last && i < n) v += dx1[i] + gcT * x1[i];
                emit(oc, b, t, first, i, v);
            }
        // r_t[n + i] = (C_t dz_t + g_t + F_t^T dlam_{t+1})[n + i] on the UNMASKED model: the gradient of the bound a held
        // control sits on, low when it equals both; free controls and the other bound get exact zeros (m <= 32 lanes)
        if ((want & kBoxBits) && L < m) {
            const int i = L;
            const bool on = bx.mask[(size_t)b * T + t] >> i & 1u;
            double s = 0.0;
            bool at_low = false;
            if (on) {
                const double *Ci = tv_at(a.C, a.sC_b, a.sC_t, b, t) + (size_t)(n + i) * d;
                const double *Ft = tv_at(a.F, a.sF_b, a.sF_t, b, t);
                s = bx.gu[((size_t)b * T + t) * m + i];
                for (int j = 0; j < d; ++j) s = fma(Ci[j], dz[j], s);
                for (int k = 0; k < n; ++k) s = fma(Ft[(size_t)k * d + n + i], dlam[k], s);
                at_low = same_bits(u[i], tv_at(bx.low, bx.slo_b, bx.slo_t, b, t)[i]);
            }
            const double vlo = ((on && at_low) ? s : 0.0) + poison, vhi = ((on && !at_low) ? s : 0.0) + poison;
            if (want >> kLo & 1u) emit(bx.olo, b, t, first, i, vlo);
            if (want >> kHi & 1u) emit(bx.ohi, b, t, first, i, vhi);
            if (want >> kRecLo & 1u) bx.Rlo[((size_t)b * T + t) * m + i] = vlo;
            if (want >> kRecHi & 1u) bx.Rhi[((size_t)b * T + t) * m + i] = vhi;
        }
        if (!LOOP) {
            if (store_factors)
                for (int r = L; r < 2 * n; r += kWaveThreads)
                    a.P[((size_t)b * T + t) * 2 * n + r] = r < n ? dlam[r] : lam[r - n];
            if (last && (want >> kCfin & 1u))
                for (int e = L; e < n * n; e += kWaveThreads) {
                    const int i = e / n, j = e % n;
                    a.o[kCfin].p[(size_t)b * a.o[kCfin].sb + e] = 0.5 * (dx1[i] * x1[j] + x1[i] * dx1[j] + gcT * x1[i] * x1[j]);
                }
            if (last && (want >> kcfin & 1u))
                for (int i = L; i < n; i += kWaveThreads) a.o[kcfin].p[(size_t)b * a.o[kcfin].sb + i] = dx1[i] + gcT * x1[i];
            if (t == 0 && (want >> kx0 & 1u))        // dx0 = dlam_0 = v~_0
                for (int i = L; i < n; i += kWaveThreads) a.o[kx0].p[(size_t)b * a.o[kx0].sb + i] = a.vt[(size_t)b * T * n + i] + poison;
            break;
        }
        __syncthreads();             // the next step overwrites the staged operands
    }
}

// ---- 5. the bounds' batch sums: tvlqr_vjp.hip's pair in double, the same fixed orders -----------------------------------
// partial[(chunk * T + t) * m + e] = sum over the chunk's instances of R[b][t][e], eight interleaved sub-sums per element
// combined in a fixed order (m <= 32).
__global__ void __launch_bounds__(kRedThreads) box_reduce_bounds_f64(const double *R, int B, int T, int m, double *partial)
{
    __shared__ double sub[kRedThreads];
    const int chunk = blockIdx.x, t = blockIdx.y, e = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int b0 = chunk * kChunk, b1 = min(B, b0 + kChunk);
    double s = 0.0;
    if (e < m)
        for (int b = b0 + g; b < b1; b += kRedThreads / 32) s += R[((size_t)b * T + t) * m + e];
    sub[threadIdx.x] = s;
    __syncthreads();
    if (g == 0 && e < m) {
        for (int k = 1; k < kRedThreads / 32; ++k) s += sub[32 * k + e];
        partial[((size_t)chunk * T + t) * m + e] = s;
    }
}

// out[slot * st + e] = sum over the chunks (and, untimed, the steps) of partial[(chunk * T + t) * m + e]: one block per
// (element, slot), 256 strided sub-sums and an LDS tree.
__global__ void __launch_bounds__(kRedThreads) box_reduce_final_f64(const double *partial, int chunks, int T, int m, bool timed,
                                                                    double *out, long st)
{
    __shared__ double sub[kRedThreads];
    const int e = blockIdx.x, slot = blockIdx.y, tid = threadIdx.x;
    const int t0 = timed ? slot : 0, nt = timed ? 1 : T, total = chunks * nt;
    double s = 0.0;
    for (int q = tid; q < total; q += kRedThreads) s += partial[((size_t)(q / nt) * T + t0 + q % nt) * m + e];
    sub[tid] = s;
    __syncthreads();
    for (int w = kRedThreads / 2; w > 0; w >>= 1) {
        if (tid < w) sub[tid] += sub[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[(size_t)slot * st + e] = sub[0];
}

// ---- workspace -------------------------------------------------------------------------------------------------------
// In doubles, every array rounded up to 64: tvlqr_vjp_f64.hip's layout (VjpPrefix, the sweeps' gains, V, vt, P, partial),
// then mask [B][T] and the second sweep's status [B] (32-bit words), gu, Rlo, Rhi [B][T][m], fhat [B][T][n],
// chat [B][T][d], vm [B][T][n].
struct Layout : VjpPrefix {
    size_t solve, V, vt, P, partial, mask, st2, gu, Rlo, Rhi, fhat, chat, vm, total;
    size_t solve_bytes;
};

Layout layout(int B, int n, int m, int T)
{
    Layout L{};
    const size_t BT = (size_t)B * T;
    size_t o = vjp_prefix(L, B, n, m, T);
    L.solve_bytes = tfmpc_tvlqr_workspace_bytes_f64(B, n, m, T);
    L.solve = o; o += up64(L.solve_bytes / sizeof(double));
    L.V = o; o += up64(BT * n * n);
    L.vt = o; o += up64(BT * n);
    L.P = o; o += up64(BT * 2 * n);
    L.partial = o; o += vjp_partial_elems(B, n, m, T);
    L.mask = o; o += up64((BT + 1) / 2);
    L.st2 = o; o += up64(((size_t)B + 1) / 2);
    L.gu = o; o += up64(BT * m);
    L.Rlo = o; o += up64(BT * m);
    L.Rhi = o; o += up64(BT * m);
    L.fhat = o; o += up64(BT * n);
    L.chat = o; o += up64(BT * (n + m));
    L.vm = o; o += up64(BT * n);
    L.total = o;
    return L;
}

}  // namespace

extern "C" {

size_t tfmpc_tvlqr_box_vjp_workspace_bytes_f64(int B, int n, int m, int T)
{
    if (B <= 0 || n <= 0 || m <= 0 || T <= 0) return 0;
    return layout(B, n, m, T).total * sizeof(double);
}

const char *tfmpc_tvlqr_box_vjp_kernel_name_f64(int n, int m, int T)
{
    (void)T;
    if (n <= 0 || m <= 0) return "invalid";
    if (!tvlqr_f64_supported(n, m)) return "unsupported";
    return tvlqr_f64_masked_kernel_name(n, m);
}

int tfmpc_tvlqr_box_vjp_f64(int B, int n, int m, int T, const double *F, long sF_b, long sF_t, const double *f, long sf_b,
                            long sf_t, const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                            const double *Cfin, long sCfin_b, const double *cfin, long scfin_b, const double *low, long slow_b,
                            long slow_t, const double *high, long shigh_b, long shigh_t, const double *states,
                            const double *actions, const double *g_states, const double *g_actions, const double *g_costs,
                            double *dF, long sdF_b, long sdF_t, double *df, long sdf_b, long sdf_t, double *dC, long sdC_b,
                            long sdC_t, double *dc, long sdc_b, long sdc_t, double *dCfin, long sdCfin_b, double *dcfin,
                            long sdcfin_b, double *dx0, long sdx0_b, double *dlow, long sdlow_b, long sdlow_t, double *dhigh,
                            long sdhigh_b, long sdhigh_t, uint32_t *clamp_mask, int32_t *status, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    if (B < 0 || n <= 0 || m <= 0 || T <= 0) return TFMPC_ERR_ARG;
    if (!tvlqr_f64_supported(n, m)) return TFMPC_ERR_UNSUPPORTED;  // n <= 32 and m <= 32: one held-set word per step
    if (B == 0) return TFMPC_OK;
    if (!F || !f || !C || !c || !states || !actions || !status) return TFMPC_ERR_ARG;
    if (!Cfin != !cfin) return TFMPC_ERR_ARG;
    if (!Cfin && (dCfin || dcfin)) return TFMPC_ERR_ARG;           // the default final cost's gradient is in dC, dc
    if (T > 65535) return TFMPC_ERR_UNSUPPORTED;                   // per-step reduction slots are one grid axis
    if ((size_t)B * (T + 1) > 0x7fffffffu) return TFMPC_ERR_UNSUPPORTED;   // fold, costates: one block per (b, t)
    if (!low || !high) return TFMPC_ERR_ARG;
    for (long s : {slow_b, slow_t, shigh_b, shigh_t, sdlow_b, sdlow_t, sdhigh_b, sdhigh_t})
        if (s < 0) return TFMPC_ERR_ARG;
    for (long s : {sF_b, sF_t, sf_b, sf_t, sC_b, sC_t, sc_b, sc_t, sCfin_b, scfin_b, sdF_b, sdF_t, sdf_b, sdf_t,
                   sdC_b, sdC_t, sdc_b, sdc_t, sdCfin_b, sdcfin_b, sdx0_b})
        if (s < 0) return TFMPC_ERR_ARG;
    const Layout L = layout(B, n, m, T);
    if (!workspace || workspace_bytes < L.total * sizeof(double)) return TFMPC_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) % sizeof(double)) return TFMPC_ERR_ARG;      // doubles are carved from it
    const int d = n + m;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *w = static_cast<double *>(workspace);

    VjpArgs a{};
    a.B = B; a.n = n; a.m = m; a.T = T;
    a.F = F; a.sF_b = sF_b; a.sF_t = sF_t;
    a.C = C; a.sC_b = sC_b; a.sC_t = sC_t;
    a.c = c; a.sc_b = sc_b; a.sc_t = sc_t;
    a.dflt = Cfin == nullptr;
    a.states = states; a.actions = actions; a.v = w + L.vm; a.gx = g_states; a.gu = g_actions; a.gc = g_costs;
    a.dS = w + L.dS; a.dA = w + L.dA; a.ct = w + L.ct; a.cT = w + L.cT;
    a.V = w + L.V; a.vt = w + L.vt;
    a.status = status; a.poison_mask = ~0;
    a.P = w + L.P;
    a.a0 = w + L.vt; a.sa0_b = (long)T * n;
    if (a.dflt) {                    // V_T: the fold's copy of C_{T-1}[:n,:n]; v_T = c_{T-1}[:n], contiguous in c
        a.Cf = w + L.Cfe; a.sCf_b = sC_b ? (long)n * n : 0;
        a.cf = c + (size_t)(T - 1) * sc_t; a.scf_b = sc_b;
    } else {
        a.Cf = Cfin; a.sCf_b = sCfin_b;
        a.cf = cfin; a.scf_b = scfin_b;
    }
    Out outs[kKinds] = {{dF, sdF_b, sdF_t}, {df, sdf_b, sdf_t}, {dC, sdC_b, sdC_t}, {dc, sdc_b, sdc_t},
                        {dCfin, sdCfin_b, 0}, {dcfin, sdcfin_b, 0}, {dx0, sdx0_b, 0}};
    for (int k = 0; k < kKinds; ++k) a.o[k] = outs[k];
    BoxArgs bx{};
    bx.low = low; bx.slo_b = slow_b; bx.slo_t = slow_t;
    bx.high = high; bx.shi_b = shigh_b; bx.shi_t = shigh_t;
    bx.mask = reinterpret_cast<uint32_t *>(w + L.mask); bx.mask_out = clamp_mask;
    bx.Rlo = w + L.Rlo; bx.Rhi = w + L.Rhi;
    bx.olo = Out{dlow, sdlow_b, sdlow_t};
    bx.ohi = Out{dhigh, sdhigh_b, sdhigh_t};
    bx.f = f; bx.sf_b = sf_b; bx.sf_t = sf_t;
    bx.fhat = w + L.fhat; bx.chat = w + L.chat; bx.gu = w + L.gu;
    int32_t *st2 = reinterpret_cast<int32_t *>(w + L.st2);

    // 1. fold
    hipLaunchKernelGGL(box_fold_f64_kernel, dim3((unsigned)((size_t)B * (T + 1))), dim3(kWaveThreads),
                       fold_smem_elems(n, m) * sizeof(double), s, a, w + L.ct, w + L.cT, w + L.Cfe, w + L.zer, bx);
    if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    // 2. adjoint sweep on the masked model: c~ per (b, t), f~ = 0 (shared), final cost (C_fin, g_T), x~0 = 0; V^m, v~ kept
    int rc = tvlqr_solve_masked_f64(B, n, m, T, F, sF_b, sF_t, w + L.zer, 0, 0, C, sC_b, sC_t, w + L.ct, (long)T * d, d, a.Cf,
                                    a.sCf_b, w + L.cT, n, w + L.zer, w + L.dS, w + L.dA, w + L.dcost, w + L.V, w + L.vt, status,
                                    bx.mask, w + L.solve, L.solve_bytes, stream);
    if (rc != TFMPC_OK) return rc;
    // 3. forward-value sweep on the masked model, backward only: (f^, c^), the true final cost; only v^m is kept
    rc = tvlqr_solve_masked_f64(B, n, m, T, F, sF_b, sF_t, bx.fhat, (long)T * n, n, C, sC_b, sC_t, bx.chat, (long)T * d, d, a.Cf,
                                a.sCf_b, a.cf, a.scf_b, nullptr, nullptr, nullptr, nullptr, nullptr, w + L.vm, st2, bx.mask,
                                w + L.solve, L.solve_bytes, stream);
    if (rc != TFMPC_OK) return rc;
    hipLaunchKernelGGL(box_status_or_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, status, st2, B);
    if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    // 4. costates and the gradients with a batch stride: per (b, t) where the output has a slot per step, per instance
    //    (in time order) where its time stride is 0; batch-shared bounds leave a record per (b, t)
    const bool reduce_F = (dF && !sdF_b) || (df && !sdf_b);
    unsigned per_step = 0, in_time = 0;
    for (int k = kF; k < kKinds; ++k) {
        if (!a.o[k].p || !a.o[k].sb) continue;
        if (k <= kc && a.o[k].st == 0 && T > 1) in_time |= 1u << k;
        else per_step |= 1u << k;
    }
    const Out bo[2] = {bx.olo, bx.ohi};
    for (int k = 0; k < 2; ++k) {
        if (!bo[k].p) continue;
        if (!bo[k].sb) per_step |= 1u << (kRecLo + k);
        else if (bo[k].st == 0 && T > 1) in_time |= 1u << (kLo + k);
        else per_step |= 1u << (kLo + k);
    }
    const size_t smem = costate_smem_elems(n, m) * sizeof(double);
    if (per_step || reduce_F) {
        hipLaunchKernelGGL(box_costate_kernel<false>, dim3((unsigned)((size_t)B * T)), dim3(kWaveThreads), smem, s, a, per_step,
                           reduce_F, bx);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    if (in_time) {
        hipLaunchKernelGGL(box_costate_kernel<true>, dim3(B), dim3(kWaveThreads), smem, s, a, in_time, false, bx);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    // 5. shared gradients: the model's, then the bounds' records -- chunks, then steps
    double *partial = w + L.partial;
    if ((rc = vjp_shared_sums<double>(a, partial, s)) != TFMPC_OK) return rc;
    const int chunks = (B + kChunk - 1) / kChunk;
    const double *rec[2] = {bx.Rlo, bx.Rhi};
    for (int k = 0; k < 2; ++k) {
        if (!bo[k].p || bo[k].sb) continue;
        hipLaunchKernelGGL(box_reduce_bounds_f64, dim3(chunks, T), dim3(kRedThreads), 0, s, rec[k], B, T, m, partial);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
        const bool timed = bo[k].st != 0;
        hipLaunchKernelGGL(box_reduce_final_f64, dim3(m, timed ? T : 1), dim3(kRedThreads), 0, s, partial, chunks, T, m, timed,
                           bo[k].p, bo[k].st);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    return TFMPC_OK;
}

}  // extern "C"
