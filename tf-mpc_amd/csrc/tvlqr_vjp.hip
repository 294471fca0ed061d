// tvlqr_vjp.hip -- gradients of a time-varying LQR solve (tfmpc_tvlqr_vjp_f32, include/tfmpc_hip.h).
//
// Given the forward trajectory z_t = [x_t; u_t] and upstream gradients on states, actions and costs, the
// vector-Jacobian product is four launches on the caller's stream:
//   1. vjp_fold_kernel    g_t = [gx_t; gu_t] + gcost_t (C_t z_t + c_t), g_T likewise with the final cost; also the
//                         adjoint's explicit final cost (a copy of C_{T-1}[:n,:n] for the default) and its zero x0 / f
//                         (fold_body, tvlqr_vjp_common.h).
//   2. the TV-LQR solve   (tfmpc_tvlqr_solve_f32, unchanged) with c~_t = g_t, c~_fin = g_T, f~ = 0, x~0 = 0 -> dz_t.
//   3. vjp_sweep_kernel   one wavefront per instance, backward in time (F_t, C_t staged in LDS per step), carrying the costates
//                         lam_t = (C_t z_t + c_t)[:n] + F_t[:, :n]^T lam_{t+1} and dlam_t (the same with dz_t, g_t); it
//                         writes every gradient whose batch stride is non-zero (dF_t = dlam_{t+1} z_t^T + lam_{t+1} dz_t^T,
//                         df_t = dlam_{t+1}, dC_t = (dz z^T + z dz^T + gcost z z^T) / 2, dc_t = dz_t + gcost_t z_t,
//                         dx0 = dlam_0) -- a time stride of 0 accumulates in the output in time order -- and, for
//                         gradients shared by the batch, stores (dlam_{t+1}, lam_{t+1}) per (b, t).
//   4. vjp_reduce_*       gradients with batch stride 0, summed over the batch in a fixed order: the kernels and the code
//                         that enqueues them are tvlqr_vjp_common.h's, shared with the double-precision gradients
//                         (tvlqr_vjp_f64.hip).
// An instance whose adjoint solve reports TFMPC_ST_NOT_PD or TFMPC_ST_SINGULAR contributes NaN (its own rows, and
// any reduction that includes it).  fp32 throughout; no scratch memory.
//
// tfmpc_tvlqr_box_vjp_f32 is the same VJP at a CONTROL-LIMITED optimum: a control that sits on a bound
// (its bits equal low's or high's) is held, du = 0, in the adjoint.  box_fold_kernel also writes the held-set word per
// (b, t) and zeroes the held entries of c~; the adjoint solve is the masked sweep (tvlqr_solve_masked_f32: the mask is
// applied as the model is loaded, no masked copy exists); box_sweep_kernel runs the costate sweep on the UNMASKED model
// and emits r_t[n + i] = (C_t dz_t + g_t + F_t^T dlam_{t+1})[n + i] of every held control into dlow or dhigh;
// box_shared_sums (tvlqr_vjp_common.h, shared with the double VJP) sums them over the batch in a fixed order.
// One vjp_impl stands behind both entries; the argument checks and the fill of VjpArgs that do not depend on the precision
// are tvlqr_vjp_common.h's (vjp_check_call, vjp_fill_base), shared with tvlqr_vjp_f64.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "lqr_kernels.h"
#include "tvlqr_kernels.h"
#include "tvlqr_vjp_common.h"

using namespace tfmpc;

namespace {

constexpr int kSweepThreads = 64;    // one wavefront per instance
constexpr int32_t kPoison = TFMPC_ST_NOT_PD | TFMPC_ST_SINGULAR;

using Out = OutT<float>;
using BoxArgs = BoxArgsT<float>;

using VjpArgs = VjpBase<float>;      // a0: the sweep's dlam_0 records [B][n]

// ---- 1. fold (fold_body, tvlqr_vjp_common.h) -------------------------------------------------------------------------
__global__ void __launch_bounds__(kWaveThreads) vjp_fold_kernel(VjpArgs a, float *ct, float *cT, float *Cfe, float *zer)
{
    fold_body<float, false>(a, ct, cT, Cfe, zer, nullptr);
}

__global__ void __launch_bounds__(kWaveThreads) box_fold_kernel(VjpArgs a, float *ct, float *cT, float *Cfe, float *zer, BoxArgs bx)
{
    fold_body<float, true>(a, ct, cT, Cfe, zer, &bx);
}

// ---- 3. costate sweep, per-instance gradients ------------------------------------------------------------------------
__device__ inline void emit(const Out &o, int b, int t, bool first, int e, float v)
{
    float *p = o.p + (size_t)b * o.sb + (size_t)t * o.st + e;
    if (o.st == 0 && !first) v += *p;   // time-shared: accumulate in time order (this lane owns element e throughout)
    *p = v;
}

template <bool BOX>
__device__ __forceinline__ void sweep_body(const VjpArgs &a, bool store_factors, const BoxArgs *bx)
{
    extern __shared__ float sm[];
    const int n = a.n, m = a.m, T = a.T, d = n + m;
    const int b = blockIdx.x, L = threadIdx.x;
    float *z = sm, *dz = z + d, *g = dz + d, *lam = g + d, *dlam = lam + n, *nl = dlam + n, *xf = nl + 2 * n,
          *dxf = xf + n, *sF = dxf + n, *sC = sF + (size_t)n * d;      // F_t [n][d], C_t [d][d + 1] staged per step
    const float poison = poison_of<float>(a.status, kPoison, b);
    const float *xT = a.states + ((size_t)b * (T + 1) + T) * n;
    const float *dxT = a.dS + ((size_t)b * (T + 1) + T) * n;
    for (int i = L; i < n; i += kSweepThreads) {
        xf[i] = xT[i] + poison;
        dxf[i] = dxT[i] + poison;
    }
    const float gcT = a.gc ? a.gc[(size_t)b * (T + 1) + T] : 0.0f;
    __syncthreads();
    // lam_T = Cf x_T + cf, dlam_T = Cf dx_T + g_T
    const float *Cf = a.Cf + (size_t)b * a.sCf_b;
    for (int r = L; r < 2 * n; r += kSweepThreads) {
        const int i = r % n;
        const bool adj = r >= n;
        const float *v = adj ? dxf : xf;
        float s = adj ? a.cT[(size_t)b * n + i] : a.cf[(size_t)b * a.scf_b + i];
        for (int j = 0; j < n; ++j) s = fmaf(Cf[(size_t)i * n + j], v[j], s);
        (adj ? dlam : lam)[i] = s;
    }
    const Out &oCf = a.o[kCfin], &ocf = a.o[kcfin];
    if (oCf.p && oCf.sb)
        for (int e = L; e < n * n; e += kSweepThreads) {
            const int i = e / n, j = e % n;
            oCf.p[(size_t)b * oCf.sb + e] = 0.5f * (dxf[i] * xf[j] + xf[i] * dxf[j] + gcT * xf[i] * xf[j]);
        }
    if (ocf.p && ocf.sb)
        for (int i = L; i < n; i += kSweepThreads) ocf.p[(size_t)b * ocf.sb + i] = dxf[i] + gcT * xf[i];
    __syncthreads();

    const Out &oF = a.o[kF], &of = a.o[kf], &oC = a.o[kC], &oc = a.o[kc];
    for (int t = T - 1; t >= 0; --t) {
        const bool first = t == T - 1;
        const float *x = a.states + ((size_t)b * (T + 1) + t) * n, *u = a.actions + ((size_t)b * T + t) * m;
        const float *dx = a.dS + ((size_t)b * (T + 1) + t) * n, *du = a.dA + ((size_t)b * T + t) * m;
        const float *gt = a.ct + ((size_t)b * T + t) * d;
        for (int i = L; i < d; i += kSweepThreads) {
            z[i] = i < n ? x[i] : u[i - n];
            dz[i] = (i < n ? dx[i] : du[i - n]) + poison;
            g[i] = gt[i];
        }
        const float gc = a.gc ? a.gc[(size_t)b * (T + 1) + t] : 0.0f;
        const float *Ft = tv_at(a.F, a.sF_b, a.sF_t, b, t), *Ct = tv_at(a.C, a.sC_b, a.sC_t, b, t);
        const float *ctv = tv_at(a.c, a.sc_b, a.sc_t, b, t);
        for (int e = L; e < n * d; e += kSweepThreads) sF[e] = Ft[e];
        for (int e = L; e < d * d; e += kSweepThreads) sC[(e / d) * (d + 1) + e % d] = Ct[e];
        __syncthreads();
        if (oF.p && oF.sb)
            for (int e = L; e < n * d; e += kSweepThreads) {
                const int i = e / d, j = e % d;
                emit(oF, b, t, first, e, fmaf(dlam[i], z[j], lam[i] * dz[j]));
            }
        if (of.p && of.sb)
            for (int i = L; i < n; i += kSweepThreads) emit(of, b, t, first, i, dlam[i]);
        if (oC.p && oC.sb)
            for (int e = L; e < d * d; e += kSweepThreads) {
                const int i = e / d, j = e % d;
                float v = 0.5f * (dz[i] * z[j] + z[i] * dz[j] + gc * z[i] * z[j]);
                if (a.dflt && first && i < n && j < n) v += 0.5f * (dxf[i] * xf[j] + xf[i] * dxf[j] + gcT * xf[i] * xf[j]);
                emit(oC, b, t, first, e, v);
            }
        if (oc.p && oc.sb)
            for (int i = L; i < d; i += kSweepThreads) {
                float v = dz[i] + gc * z[i];
                if (a.dflt && first && i < n) v += dxf[i] + gcT * xf[i];
                emit(oc, b, t, first, i, v);
            }
        if (store_factors)
            for (int r = L; r < 2 * n; r += kSweepThreads)
                a.P[((size_t)b * T + t) * 2 * n + r] = r < n ? dlam[r] : lam[r - n];
        // lam_t = (C_t z_t + c_t)[:n] + F_t[:, :n]^T lam_{t+1};  dlam_t = (C_t dz_t + g_t)[:n] + F_t[:, :n]^T dlam_{t+1}
        // (BOX: m more rows in the same pass, r_t[n + i] = (C_t dz_t + g_t + F_t^T dlam_{t+1})[n + i] -- the gradient of the bound
        // a held control sits on, low when it equals both; free controls and the other bound get 0)
        const uint32_t held = BOX ? bx->mask[(size_t)b * T + t] : 0u;
        for (int r = L; r < 2 * n + (BOX ? m : 0); r += kSweepThreads) {
            if (BOX && r >= 2 * n) {
                const int i = r - 2 * n;
                float *rec = bx->Rlo + ((size_t)b * T + t) * m + i;
                const bool on = held >> i & 1u;
                const float *Ci = sC + (size_t)(n + i) * (d + 1);
                float s = *rec;                          // the fold's unmasked g_u
                for (int j = 0; j < d; ++j) s = fmaf(Ci[j], dz[j], s);
                for (int k = 0; k < n; ++k) s = fmaf(sF[(size_t)k * d + n + i], dlam[k], s);
                const bool at_low = same_bits(u[i], tv_at(bx->low, bx->slo_b, bx->slo_t, b, t)[i]);
                const float vlo = ((on && at_low) ? s : 0.0f) + poison, vhi = ((on && !at_low) ? s : 0.0f) + poison;
                if (bx->olo.p) {
                    if (bx->olo.sb) emit(bx->olo, b, t, first, i, vlo);
                    else *rec = vlo;
                }
                if (bx->ohi.p) {
                    if (bx->ohi.sb) emit(bx->ohi, b, t, first, i, vhi);
                    else bx->Rhi[((size_t)b * T + t) * m + i] = vhi;
                }
                continue;
            }
            const int i = r % n;
            const bool adj = r >= n;
            const float *v = adj ? dz : z, *l = adj ? dlam : lam;
            const float *Ci = sC + (size_t)i * (d + 1);
            float s = adj ? g[i] : ctv[i];
            for (int j = 0; j < d; ++j) s = fmaf(Ci[j], v[j], s);
            for (int k = 0; k < n; ++k) s = fmaf(sF[(size_t)k * d + i], l[k], s);
            nl[r] = s;
        }
        __syncthreads();
        for (int r = L; r < 2 * n; r += kSweepThreads) (r < n ? lam : dlam)[r % n] = nl[r];
        __syncthreads();
    }
    const Out &ox = a.o[kx0];
    if (ox.p)
        for (int i = L; i < n; i += kSweepThreads) {
            if (ox.sb) ox.p[(size_t)b * ox.sb + i] = dlam[i];
            else a.a0[(size_t)b * n + i] = dlam[i];
        }
}

__global__ void __launch_bounds__(kSweepThreads) vjp_sweep_kernel(VjpArgs a, bool store_factors)
{
    sweep_body<false>(a, store_factors, nullptr);
}

__global__ void __launch_bounds__(kSweepThreads) box_sweep_kernel(VjpArgs a, bool store_factors, BoxArgs bx)
{
    sweep_body<true>(a, store_factors, &bx);
}

// ---- launch helpers --------------------------------------------------------------------------------------------------
size_t fold_smem_bytes(int n, int m) { return fold_smem_elems(n, m) * sizeof(float); }

size_t sweep_smem_bytes(int n, int m)
{
    const size_t d = n + m;
    return (3 * d + 6 * (size_t)n + (size_t)n * d + d * (d + 1)) * sizeof(float);
}

// ---- workspace (tvlqr_vjp_common.h) ----------------------------------------------------------------------------------
struct Layout : VjpPrefix {
    size_t solve, P, Pf, partial, total;     // offsets in floats
    size_t solve_bytes;
};

Layout layout(int B, int n, int m, int T)
{
    Layout L{};
    size_t o = vjp_prefix(L, B, n, m, T);
    L.solve_bytes = tfmpc_tvlqr_workspace_bytes(B, n, m, T);
    L.solve = o; o += up64((L.solve_bytes + 3) / 4);
    L.P = o; o += up64((size_t)B * T * 2 * n);
    L.Pf = o; o += up64((size_t)B * n);
    L.partial = o; o += vjp_partial_elems(B, n, m, T);
    L.total = o;
    return L;
}

struct BoxLayout { size_t mask, Rlo, Rhi, total; };   // offsets in floats, after the plain VJP's workspace

BoxLayout box_layout(int B, int n, int m, int T)
{
    BoxLayout L{};
    size_t o = layout(B, n, m, T).total;
    L.mask = o; o += up64((size_t)B * T);
    L.Rlo = o; o += up64((size_t)B * T * m);
    L.Rhi = o; o += up64((size_t)B * T * m);
    L.total = o;
    return L;
}

// Both entries; box: the control-limited one's extra arguments.  The checks and the fill of VjpArgs that do not depend
// on the precision are tvlqr_vjp_common.h's.
int vjp_impl(const VjpCall<float> &c, const BoxCall<float> *box)
{
    const int B = c.B, n = c.n, m = c.m, T = c.T, d = n + m;
    if (B < 0 || n <= 0 || m <= 0 || T <= 0) return TFMPC_ERR_ARG;
    if (!tvlqr_mfma_supported(n, m) && tvlqr_generic_smem_bytes(n, m) > kMaxLdsBytes) return TFMPC_ERR_UNSUPPORTED;
    if (B == 0) return TFMPC_OK;
    const bool fits = sweep_smem_bytes(n, m) <= kMaxLdsBytes && fold_smem_bytes(n, m) <= kMaxLdsBytes &&
                      !(box && m > 32);                            // one held-set word per step
    if (const int rc = vjp_check_call(c, box, fits); rc != TFMPC_OK) return rc;
    const Layout L = layout(B, n, m, T);
    const BoxLayout XL = box ? box_layout(B, n, m, T) : BoxLayout{};
    if (!c.workspace || c.workspace_bytes < (box ? XL.total : L.total) * sizeof(float)) return TFMPC_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    float *w = static_cast<float *>(c.workspace);

    VjpArgs a{};
    vjp_fill_base(a, c, w, L);
    a.poison_mask = kPoison;
    a.P = w + L.P; a.a0 = w + L.Pf; a.sa0_b = n;
    BoxArgs bx{};
    if (box) box_fill(bx, *box, reinterpret_cast<uint32_t *>(w + XL.mask), w + XL.Rlo, w + XL.Rhi);

    // 1. fold
    {
        const size_t smem = fold_smem_bytes(n, m);
        const dim3 grid((unsigned)((size_t)B * (T + 1)));
        if (box) {
            if (!allow_lds(box_fold_kernel, smem)) return TFMPC_ERR_LAUNCH;
            hipLaunchKernelGGL(box_fold_kernel, grid, dim3(kWaveThreads), smem, s, a, w + L.ct, w + L.cT, w + L.Cfe, w + L.zer, bx);
        } else {
            if (!allow_lds(vjp_fold_kernel, smem)) return TFMPC_ERR_LAUNCH;
            hipLaunchKernelGGL(vjp_fold_kernel, grid, dim3(kWaveThreads), smem, s, a, w + L.ct, w + L.cT, w + L.Cfe, w + L.zer);
        }
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    // 2. adjoint solve: c~ per (b, t), f~ = 0 (shared), explicit final cost, x~0 = 0
    {
        int rc;
        if (box)                     // the held controls taken out of the model as it is loaded
            rc = tvlqr_solve_masked_f32(B, n, m, T, c.F, c.sF_b, c.sF_t, w + L.zer, 0, 0, c.C, c.sC_b, c.sC_t, w + L.ct, (long)T * d, d,
                                        a.Cf, a.sCf_b, w + L.cT, n, w + L.zer, w + L.dS, w + L.dA, w + L.dcost, c.status,
                                        bx.mask, w + L.solve, L.solve_bytes, c.stream);
        else
            rc = tfmpc_tvlqr_solve_f32(B, n, m, T, c.F, c.sF_b, c.sF_t, w + L.zer, 0, 0, c.C, c.sC_b, c.sC_t, w + L.ct, (long)T * d, d,
                                       a.Cf, a.sCf_b, w + L.cT, n, w + L.zer, w + L.dS, w + L.dA, w + L.dcost, nullptr,
                                       nullptr, nullptr, nullptr, nullptr, c.status, w + L.solve, L.solve_bytes, c.stream);
        if (rc != TFMPC_OK) return rc;
    }
    // 3. sweep
    const bool reduce_F = (c.dF && !c.sdF_b) || (c.df && !c.sdf_b);
    {
        const size_t smem = sweep_smem_bytes(n, m);
        if (box) {
            if (!allow_lds(box_sweep_kernel, smem)) return TFMPC_ERR_LAUNCH;
            hipLaunchKernelGGL(box_sweep_kernel, dim3(B), dim3(kSweepThreads), smem, s, a, reduce_F, bx);
        } else {
            if (!allow_lds(vjp_sweep_kernel, smem)) return TFMPC_ERR_LAUNCH;
            hipLaunchKernelGGL(vjp_sweep_kernel, dim3(B), dim3(kSweepThreads), smem, s, a, reduce_F);
        }
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    // 4. shared gradients: the model's, then the bounds' from the sweep's records
    float *partial = w + L.partial;
    if (const int rc = vjp_shared_sums<float>(a, partial, s); rc != TFMPC_OK) return rc;
    return box ? box_shared_sums<float>(bx, B, T, m, partial, s) : TFMPC_OK;
}

}  // namespace

extern "C" {

size_t tfmpc_tvlqr_vjp_workspace_bytes(int B, int n, int m, int T)
{
    if (B <= 0 || n <= 0 || m <= 0 || T <= 0) return 0;
    return layout(B, n, m, T).total * sizeof(float);
}

int tfmpc_tvlqr_vjp_f32(int B, int n, int m, int T, const float *F, long sF_b, long sF_t, const float *f, long sf_b, long sf_t,
                        const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t, const float *Cfin,
                        long sCfin_b, const float *cfin, long scfin_b, const float *states, const float *actions,
                        const float *g_states, const float *g_actions, const float *g_costs, float *dF, long sdF_b, long sdF_t,
                        float *df, long sdf_b, long sdf_t, float *dC, long sdC_b, long sdC_t, float *dc, long sdc_b, long sdc_t,
                        float *dCfin, long sdCfin_b, float *dcfin, long sdcfin_b, float *dx0, long sdx0_b, int32_t *status,
                        void *workspace, size_t workspace_bytes, void *stream)
{
    return vjp_impl({B, n, m, T, F, sF_b, sF_t, f, sf_b, sf_t, C, sC_b, sC_t, c, sc_b, sc_t, Cfin, sCfin_b, cfin, scfin_b, states,
                     actions, g_states, g_actions, g_costs, dF, sdF_b, sdF_t, df, sdf_b, sdf_t, dC, sdC_b, sdC_t, dc, sdc_b, sdc_t,
                     dCfin, sdCfin_b, dcfin, sdcfin_b, dx0, sdx0_b, status, workspace, workspace_bytes, stream},
                    nullptr);
}

size_t tfmpc_tvlqr_box_vjp_workspace_bytes(int B, int n, int m, int T)
{
    if (B <= 0 || n <= 0 || m <= 0 || T <= 0) return 0;
    return box_layout(B, n, m, T).total * sizeof(float);
}

const char *tfmpc_tvlqr_box_vjp_kernel_name(int n, int m, int T)
{
    (void)T;
    if (n <= 0 || m <= 0) return "invalid";
    if (tvlqr_mfma_supported(n, m)) return (n == 16 && m == 8) ? "tv_masked_16x8" : "tv_masked_16x8 (zero-padded)";
    if (m > 32 || tvlqr_generic_smem_bytes(n, m) > kMaxLdsBytes || sweep_smem_bytes(n, m) > kMaxLdsBytes) return "unsupported";
    return "tv_masked_generic_wave";
}

int tfmpc_tvlqr_box_vjp_f32(int B, int n, int m, int T, const float *F, long sF_b, long sF_t, const float *f, long sf_b, long sf_t,
                            const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t, const float *Cfin,
                            long sCfin_b, const float *cfin, long scfin_b, const float *low, long slow_b, long slow_t,
                            const float *high, long shigh_b, long shigh_t, const float *states, const float *actions,
                            const float *g_states, const float *g_actions, const float *g_costs, float *dF, long sdF_b,
                            long sdF_t, float *df, long sdf_b, long sdf_t, float *dC, long sdC_b, long sdC_t, float *dc,
                            long sdc_b, long sdc_t, float *dCfin, long sdCfin_b, float *dcfin, long sdcfin_b, float *dx0,
                            long sdx0_b, float *dlow, long sdlow_b, long sdlow_t, float *dhigh, long sdhigh_b, long sdhigh_t,
                            uint32_t *clamp_mask, int32_t *status, void *workspace, size_t workspace_bytes, void *stream)
{
    const BoxCall<float> box{low, slow_b, slow_t, high, shigh_b, shigh_t, dlow, sdlow_b, sdlow_t, dhigh, sdhigh_b, sdhigh_t, clamp_mask};
    return vjp_impl({B, n, m, T, F, sF_b, sF_t, f, sf_b, sf_t, C, sC_b, sC_t, c, sc_b, sc_t, Cfin, sCfin_b, cfin, scfin_b, states,
                     actions, g_states, g_actions, g_costs, dF, sdF_b, sdF_t, df, sdf_b, sdf_t, dC, sdC_b, sdC_t, dc, sdc_b, sdc_t,
                     dCfin, sdCfin_b, dcfin, sdcfin_b, dx0, sdx0_b, status, workspace, workspace_bytes, stream},
                    &box);
}

}  // extern "C"
