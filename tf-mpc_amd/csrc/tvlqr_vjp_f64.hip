// tvlqr_vjp_f64.hip -- gradients of the DOUBLE-PRECISION time-varying LQR solve (tfmpc_tvlqr_vjp_f64,
// include/tfmpc_hip.h).
//
// The contract is tfmpc_tvlqr_vjp_f32's (tvlqr_vjp.hip); the costates are NOT that file's.  There they
// come from the open-loop recursion lam_t = (C_t z_t + c_t)[:n] + F_t[:, :n]^T lam_{t+1}, which multiplies rounding
// error by the spectral radius of F_x at every step -- on the unscaled models the double path exists for, fp64 through
// that recursion is wrong in the second digit at T = 20.  Here they are the gradient of the value function on the
// optimal trajectory,
//   lam_{t+1}  = V_{t+1} x_{t+1}  + v_{t+1}      (v: the FORWARD solve's, an input of the call)
//   dlam_{t+1} = V_{t+1} dx_{t+1} + v~_{t+1}     (V, v~: the ADJOINT solve's; V does not depend on linear terms)
// with V_T = C_fin, v_T = c_fin, v~_T = g_T, which is closed-loop: nothing grows, and no step depends on another.
// Five kinds of launches on the caller's stream:
//   1. vjp_fold_kernel      g_t = [gx_t; gu_t] + gcost_t (C_t z_t + c_t), g_T likewise with the final cost; the adjoint's
//                           explicit final cost (a copy of C_{T-1}[:n,:n] for the default) and its zero x0 / f.
//   2. the TV-LQR solve     (tfmpc_tvlqr_solve_f64) with c~_t = g_t, c~_fin = g_T, f~ = 0, x~0 = 0 -> dz_t, and V, v~ into
//                           the workspace.
//   3. vjp_costate_kernel   one wavefront per (b, t): V_{t+1} staged once in LDS serves both matrix-vector products; then
//                           dF_t = dlam_{t+1} z_t^T + lam_{t+1} dz_t^T, df_t = dlam_{t+1}, dC_t, dc_t (at t = T - 1 with the
//                           final-cost terms), dx0 = v~_0, and for gradients shared by the batch the record
//                           (dlam_{t+1}, lam_{t+1}) per (b, t).  It reads V, never F_t or C_t.  <LOOP = true>: one wavefront
//                           per instance walks t = T - 1 .. 0 for the per-instance outputs whose TIME stride is 0, so that
//                           one lane owns an element and adds its terms in time order (no atomics).
//   4. vjp_reduce_*         gradients with batch stride 0, summed over the batch in a fixed order: the kernels and the code
//                           that enqueues them are tvlqr_vjp_common.h's, shared with tvlqr_vjp.hip (as is the fold's body).
// An instance whose adjoint solve sets a status bit contributes NaN (its own rows, and every batch sum that includes it).
// The build is -ffp-contract=off: every fused multiply-add is a written fma().  No scratch memory.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "tvlqr_kernels.h"
#include "tvlqr_vjp_common.h"

using namespace tfmpc;

namespace {

using Out = OutT<double>;

struct VjpArgs : VjpBase<double> {
    const double *v;                 // the forward solve's v[B][T][n]
    const double *V, *vt;            // the adjoint solve's V[B][T][n][n], v~[B][T][n] (v~_0: the base's a0)
};

// ---- 1. fold (fold_body, tvlqr_vjp_common.h) -------------------------------------------------------------------------
__global__ void __launch_bounds__(kWaveThreads) vjp_fold_kernel(VjpArgs a, double *ct, double *cT, double *Cfe, double *zer)
{
    fold_body<double, false>(a, ct, cT, Cfe, zer, nullptr);
}

// ---- 3. value-function costates and per-instance gradients -----------------------------------------------------------
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

// KEEP IN STEP: tvlqr_box_vjp_f64.hip's box_costate_kernel is this kernel with the bounds' gradient added (a copy, so
// that this file's kernels keep their text).  A change to the arithmetic here belongs there too: with no
// control held the two must give the same bits (tests/test_tvlqr_box_grad_f64_gpu.py).
// want: bit k = emit output k here.  LOOP = false: grid B T, block (b, t), every emitted output has its own slot per
// step (or T == 1).  LOOP = true: grid B, the block walks the steps backwards and accumulates in the output.
template <bool LOOP>
__global__ void __launch_bounds__(kWaveThreads) vjp_costate_kernel(VjpArgs a, unsigned want, bool store_factors)
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

// ---- workspace (tvlqr_vjp_common.h) ----------------------------------------------------------------------------------
struct Layout : VjpPrefix {
    size_t solve, V, vt, P, partial, total;  // offsets in doubles
    size_t solve_bytes;
};

Layout layout(int B, int n, int m, int T)
{
    Layout L{};
    size_t o = vjp_prefix(L, B, n, m, T);
    L.solve_bytes = tfmpc_tvlqr_workspace_bytes_f64(B, n, m, T);
    L.solve = o; o += up64(L.solve_bytes / sizeof(double));
    L.V = o; o += up64((size_t)B * T * n * n);
    L.vt = o; o += up64((size_t)B * T * n);
    L.P = o; o += up64((size_t)B * T * 2 * n);
    L.partial = o; o += vjp_partial_elems(B, n, m, T);
    L.total = o;
    return L;
}

}  // namespace

extern "C" {

size_t tfmpc_tvlqr_vjp_workspace_bytes_f64(int B, int n, int m, int T)
{
    if (B <= 0 || n <= 0 || m <= 0 || T <= 0) return 0;
    return layout(B, n, m, T).total * sizeof(double);
}

int tfmpc_tvlqr_vjp_f64(int B, int n, int m, int T, const double *F, long sF_b, long sF_t, const double *f, long sf_b,
                        long sf_t, const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                        const double *Cfin, long sCfin_b, const double *cfin, long scfin_b, const double *states,
                        const double *actions, const double *v, const double *g_states, const double *g_actions,
                        const double *g_costs, double *dF, long sdF_b, long sdF_t, double *df, long sdf_b, long sdf_t,
                        double *dC, long sdC_b, long sdC_t, double *dc, long sdc_b, long sdc_t, double *dCfin,
                        long sdCfin_b, double *dcfin, long sdcfin_b, double *dx0, long sdx0_b, int32_t *status,
                        void *workspace, size_t workspace_bytes, void *stream)
{
    if (B < 0 || n <= 0 || m <= 0 || T <= 0) return TFMPC_ERR_ARG;
    if (!tvlqr_f64_supported(n, m)) return TFMPC_ERR_UNSUPPORTED;
    if (B == 0) return TFMPC_OK;
    if (!F || !f || !C || !c || !states || !actions || !v || !status) return TFMPC_ERR_ARG;
    if (!Cfin != !cfin) return TFMPC_ERR_ARG;
    if (!Cfin && (dCfin || dcfin)) return TFMPC_ERR_ARG;           // the default final cost's gradient is in dC, dc
    if (T > 65535) return TFMPC_ERR_UNSUPPORTED;                   // per-step reduction slots are one grid axis
    if ((size_t)B * (T + 1) > 0x7fffffffu) return TFMPC_ERR_UNSUPPORTED;   // fold, costates: one block per (b, t)
    for (long s : {sF_b, sF_t, sf_b, sf_t, sC_b, sC_t, sc_b, sc_t, sCfin_b, scfin_b, sdF_b, sdF_t, sdf_b, sdf_t,
                   sdC_b, sdC_t, sdc_b, sdc_t, sdCfin_b, sdcfin_b, sdx0_b})
        if (s < 0) return TFMPC_ERR_ARG;
    const Layout L = layout(B, n, m, T);
    if (!workspace || workspace_bytes < L.total * sizeof(double)) return TFMPC_ERR_WORKSPACE;
    const int d = n + m;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *w = static_cast<double *>(workspace);

    VjpArgs a{};
    a.B = B; a.n = n; a.m = m; a.T = T;
    a.C = C; a.sC_b = sC_b; a.sC_t = sC_t;
    a.c = c; a.sc_b = sc_b; a.sc_t = sc_t;
    a.dflt = Cfin == nullptr;
    a.states = states; a.actions = actions; a.v = v; a.gx = g_states; a.gu = g_actions; a.gc = g_costs;
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

    // 1. fold
    hipLaunchKernelGGL(vjp_fold_kernel, dim3((unsigned)((size_t)B * (T + 1))), dim3(kWaveThreads),
                       fold_smem_elems(n, m) * sizeof(double), s, a, w + L.ct, w + L.cT, w + L.Cfe, w + L.zer);
    if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    // 2. adjoint solve: c~ per (b, t), f~ = 0 (shared), explicit final cost, x~0 = 0; V and v~ are kept
    {
        const int rc = tfmpc_tvlqr_solve_f64(B, n, m, T, F, sF_b, sF_t, w + L.zer, 0, 0, C, sC_b, sC_t, w + L.ct, (long)T * d, d,
                                             a.Cf, a.sCf_b, w + L.cT, n, w + L.zer, w + L.dS, w + L.dA, w + L.dcost, nullptr,
                                             nullptr, w + L.V, w + L.vt, nullptr, status, w + L.solve, L.solve_bytes, stream);
        if (rc != TFMPC_OK) return rc;
    }
    // 3. costates and the gradients with a batch stride: per (b, t) where the output has a slot per step, per instance
    //    (in time order) where its time stride is 0
    const bool reduce_F = (dF && !sdF_b) || (df && !sdf_b);
    unsigned per_step = 0, in_time = 0;
    for (int k = kF; k < kKinds; ++k) {
        if (!a.o[k].p || !a.o[k].sb) continue;
        if (k <= kc && a.o[k].st == 0 && T > 1) in_time |= 1u << k;
        else per_step |= 1u << k;
    }
    const size_t smem = costate_smem_elems(n, m) * sizeof(double);
    if (per_step || reduce_F) {
        hipLaunchKernelGGL(vjp_costate_kernel<false>, dim3((unsigned)((size_t)B * T)), dim3(kWaveThreads), smem, s, a, per_step,
                           reduce_F);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    if (in_time) {
        hipLaunchKernelGGL(vjp_costate_kernel<true>, dim3(B), dim3(kWaveThreads), smem, s, a, in_time, false);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    // 4. shared gradients
    return vjp_shared_sums<double>(a, w + L.partial, s);
}

}  // extern "C"
