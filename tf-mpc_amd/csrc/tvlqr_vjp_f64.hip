// tvlqr_vjp_f64.hip -- gradients of the DOUBLE-PRECISION time-varying LQR solve, plain and control-limited
// (tfmpc_tvlqr_vjp_f64, tfmpc_tvlqr_box_vjp_f64, include/tfmpc_hip.h).
//
// The contracts are tfmpc_tvlqr_vjp_f32's and tfmpc_tvlqr_box_vjp_f32's (tvlqr_vjp.hip), and as there
// one vjp_f64_impl stands behind both entries; the costates are NOT that file's.  There they come from the open-loop
// recursion lam_t = (C_t z_t + c_t)[:n] + F_t[:, :n]^T lam_{t+1}, which multiplies rounding error by the spectral radius
// of F_x at every step -- on the unscaled models the double path exists for, fp64 through that recursion is wrong in the
// second digit at T = 20.  Here they are the gradient of the value function on the optimal trajectory,
//   lam_{t+1}  = V_{t+1} x_{t+1}  + v_{t+1}      (v: the FORWARD solve's, an input of the plain call)
//   dlam_{t+1} = V_{t+1} dx_{t+1} + v~_{t+1}     (V, v~: the ADJOINT solve's; V does not depend on linear terms)
// with V_T = C_fin, v_T = c_fin, v~_T = g_T, which is closed-loop: nothing grows, and no step depends on another.
// The plain VJP, launches on the caller's stream (no allocation, no sync, no atomics):
//   1. vjp_fold_kernel      g_t = [gx_t; gu_t] + gcost_t (C_t z_t + c_t), g_T likewise with the final cost; the adjoint's
//                           explicit final cost (a copy of C_{T-1}[:n,:n] for the default) and its zero x0 / f.
//   2. the TV-LQR solve     (tfmpc_tvlqr_solve_f64) with c~_t = g_t, c~_fin = g_T, f~ = 0, x~0 = 0 -> dz_t, and V, v~ into
//                           the workspace.
//   3. vjp_costate_kernel   one wavefront per (b, t): V_{t+1} staged once in LDS serves both matrix-vector products; then
//                           dF_t = dlam_{t+1} z_t^T + lam_{t+1} dz_t^T, df_t = dlam_{t+1}, dC_t, dc_t (at t = T - 1 with the
//                           final-cost terms), dx0 = v~_0, and for gradients shared by the batch the record
//                           (dlam_{t+1}, lam_{t+1}) per (b, t).  It reads V, never F_t or C_t.  <LOOP = true>: one wavefront
//                           per instance walks t = T - 1 .. 0 for the per-instance outputs whose TIME stride is 0, so that
//                           one lane owns an element and adds its terms in time order.
//   4. vjp_reduce_*         gradients with batch stride 0, summed over the batch in a fixed order: the kernels and the code
//                           that enqueues them are tvlqr_vjp_common.h's, shared with tvlqr_vjp.hip (as is the fold's body).
// The control-limited VJP: a control whose bits equal low's or high's is held, du = 0 in the adjoint, and the costates are
// those of the REDUCED problem, held controls fixed at their bounds and free ones optimised:
//   lam_{t+1}  = V^m_{t+1} x_{t+1}  + v^m_{t+1}
//   dlam_{t+1} = V^m_{t+1} dx_{t+1} + v~_{t+1}
// V^m: the Riccati sequence of the masked model (the adjoint solve produces it); v~: the masked adjoint solve's v; v^m:
// the v of the same masked model with the forward's reduced linear terms f^_t = f_t + F_t[:, n + H_t] u_{H_t},
// c^_t = c_t + C_t[:, n + H_t] u_{H_t} and the true final cost.  Nothing the forward exports gives v^m, so a second
// masked backward sweep computes it.  Its launches:
//   1. box_fold_f64_kernel  fold_body<double, true> (g_t, the held-set word, c~ with the held entries zeroed, the unmasked
//                           g_u), and f^_t, c^_t per (b, t).
//   2. the masked sweep     (tvlqr_solve_masked_f64) with c~ = g, f~ = 0, x~0 = 0, final cost (C_fin, g_T) -> dz, V^m, v~;
//                           then once more, backward only, with (f^, c^) and the true final cost -> v^m;
//                           box_status_or_kernel: the status is the OR of both sweeps'.
//   3. vjp_costate_kernel   <BOX = true>: the same body, in which lane i < m of a held control also forms
//                           r_t[n + i] = (C_t dz_t + g_t + F_t^T dlam_{t+1})[n + i], the gradient of the bound the control
//                           sits on (low when it equals both); free controls and the other bound get exact zeros.
//   4. the batch sums       vjp_shared_sums<double> for the model's gradients, box_shared_sums<double> for the bounds'.
// Launches 1 and 3 - 4 of the plain VJP can also be enqueued from outside (tvlqr_vjp_f64_fold_launch,
// tvlqr_vjp_f64_costates_launch; tvlqr_vjp_common.h): the segmented adjoint of the time-parallel solve brings its own v~, dx,
// du and the forward's V (tvlqr_vjp_time_parallel_f64.hip).
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
    const double *v;                 // the forward solve's v[B][T][n] (control-limited: v^m, the forward-value sweep's)
    const double *V, *vt;            // the adjoint solve's V[B][T][n][n], v~[B][T][n] (v~_0: the base's a0)
};

struct BoxArgs : BoxArgsT<double> {
    const double *f;                 // the fold's second job: f^ [B][T][n], c^ [B][T][d]
    long sf_b, sf_t;
    double *fhat, *chat;
    double *gu;                      // [B][T][m]: the fold's unmasked g_u
};

// ---- 1. fold (fold_body, tvlqr_vjp_common.h) -------------------------------------------------------------------------
__global__ void __launch_bounds__(kWaveThreads) vjp_fold_kernel(VjpArgs a, double *ct, double *cT, double *Cfe, double *zer)
{
    fold_body<double, false>(a, ct, cT, Cfe, zer, nullptr);
}

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

// ---- 2. the status of the control-limited call: both sweeps' -----------------------------------------------------------
__global__ void box_status_or_kernel(int32_t *status, const int32_t *second, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) status[b] |= second[b];
}

// ---- 3. value-function costates, per-instance gradients, the bounds' gradients ---------------------------------------
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

// bits of the costate kernel's `want` beyond the model's kinds: dlow / dhigh written in place, or as a record per (b, t)
enum BoxKind { kLo = kKinds, kHi, kRecLo, kRecHi };
constexpr unsigned kBoxBits = 1u << kLo | 1u << kHi | 1u << kRecLo | 1u << kRecHi;

// The costate kernel's last argument: nothing for the plain VJP, the bounds' operands for the control-limited one.  (One
// kernel template, not a shared device function under two named kernels: that form changes the scalar code of all four
// instantiations)
template <bool BOX>
struct BoxTail {};
template <>
struct BoxTail<true> : BoxArgs {};

// want: bit k = emit output k here.  LOOP = false: grid B T, block (b, t), every emitted output has its own slot per
// step (or T == 1).  LOOP = true: grid B, the block walks the steps backwards and accumulates in the output.
// BOX: lane i < m of a held control also forms the gradient of the bound it sits on.
template <bool LOOP, bool BOX>
__global__ void __launch_bounds__(kWaveThreads) vjp_costate_kernel(VjpArgs a, unsigned want, bool store_factors, BoxTail<BOX> bx)
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
        if constexpr (BOX)
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

// Per (b, t) where the output has a slot per step, per instance (in time order) where its time stride is 0.
template <bool BOX>
int launch_costates(const VjpArgs &a, unsigned per_step, unsigned in_time, bool reduce_F, const BoxTail<BOX> &bx, hipStream_t s)
{
    const size_t smem = costate_smem_elems(a.n, a.m) * sizeof(double);
    if (per_step || reduce_F) {
        hipLaunchKernelGGL((vjp_costate_kernel<false, BOX>), dim3((unsigned)((size_t)a.B * a.T)), dim3(kWaveThreads), smem, s, a,
                           per_step, reduce_F, bx);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    if (in_time) {
        hipLaunchKernelGGL((vjp_costate_kernel<true, BOX>), dim3(a.B), dim3(kWaveThreads), smem, s, a, in_time, false, bx);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    return TFMPC_OK;
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

// The control-limited VJP's tail, in doubles after the plain VJP's workspace, every array rounded up to 64: mask [B][T]
// and the second sweep's status [B] (32-bit words), gu, Rlo, Rhi [B][T][m], fhat [B][T][n], chat [B][T][d], vm [B][T][n].
struct BoxLayout { size_t mask, st2, gu, Rlo, Rhi, fhat, chat, vm, total; };

BoxLayout box_layout(int B, int n, int m, int T)
{
    BoxLayout L{};
    const size_t BT = (size_t)B * T;
    size_t o = layout(B, n, m, T).total;
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

// VjpArgs of a call whose workspace w starts with VjpPrefix: the forward's v (or v^m), the adjoint's V and v~, the records
VjpArgs make_args(const VjpCall<double> &c, double *w, const VjpPrefix &L, const double *v, const double *V, const double *vt, double *P)
{
    VjpArgs a{};
    vjp_fill_base<double>(a, c, w, L);
    a.v = v;
    a.V = V; a.vt = vt;
    a.poison_mask = ~0;
    a.P = P;
    a.a0 = const_cast<double *>(vt); a.sa0_b = (long)c.T * c.n;
    return a;
}

// dF or df shared by the batch: the costate kernel leaves a record (dlam_{t+1}, lam_{t+1}) per (b, t)
bool wants_records(const VjpCall<double> &c) { return (c.dF && !c.sdF_b) || (c.df && !c.sdf_b); }

// The model's gradients with a batch stride: emitted per (b, t), or per instance in time order (time stride 0)
void model_wants(const VjpArgs &a, unsigned &per_step, unsigned &in_time)
{
    for (int k = kF; k < kKinds; ++k) {
        if (!a.o[k].p || !a.o[k].sb) continue;
        if (k <= kc && a.o[k].st == 0 && a.T > 1) in_time |= 1u << k;
        else per_step |= 1u << k;
    }
}

// Both entries.  Plain (box == NULL): v is the forward solve's, from the caller.  Control-limited: v is not given; the
// second masked sweep computes v^m.  The checks and the fill of VjpArgs that do not depend on the precision are
// tvlqr_vjp_common.h's.
int vjp_f64_impl(const VjpCall<double> &c, const double *v, const BoxCall<double> *box)
{
    const int B = c.B, n = c.n, m = c.m, T = c.T, d = n + m;
    if (B < 0 || n <= 0 || m <= 0 || T <= 0) return TFMPC_ERR_ARG;
    if (!tvlqr_f64_supported(n, m)) return TFMPC_ERR_UNSUPPORTED;  // n <= 32 and m <= 32: one held-set word per step
    if (B == 0) return TFMPC_OK;
    if (!box && !v) return TFMPC_ERR_ARG;
    if (const int rc = vjp_check_call(c, box, true); rc != TFMPC_OK) return rc;
    const Layout L = layout(B, n, m, T);
    const BoxLayout XL = box ? box_layout(B, n, m, T) : BoxLayout{};
    if (!c.workspace || c.workspace_bytes < (box ? XL.total : L.total) * sizeof(double)) return TFMPC_ERR_WORKSPACE;
    if (box && reinterpret_cast<uintptr_t>(c.workspace) % sizeof(double)) return TFMPC_ERR_ARG;    // doubles are carved from it
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    double *w = static_cast<double *>(c.workspace);

    const VjpArgs a = make_args(c, w, L, box ? w + XL.vm : v, w + L.V, w + L.vt, w + L.P);
    BoxTail<true> bx{};
    if (box) {
        box_fill<double>(bx, *box, reinterpret_cast<uint32_t *>(w + XL.mask), w + XL.Rlo, w + XL.Rhi);
        bx.f = c.f; bx.sf_b = c.sf_b; bx.sf_t = c.sf_t;
        bx.fhat = w + XL.fhat; bx.chat = w + XL.chat; bx.gu = w + XL.gu;
    }

    // 1. fold
    const dim3 fold_grid((unsigned)((size_t)B * (T + 1)));
    const size_t fold_smem = fold_smem_elems(n, m) * sizeof(double);
    if (box)
        hipLaunchKernelGGL(box_fold_f64_kernel, fold_grid, dim3(kWaveThreads), fold_smem, s, a, w + L.ct, w + L.cT, w + L.Cfe,
                           w + L.zer, bx);
    else
        hipLaunchKernelGGL(vjp_fold_kernel, fold_grid, dim3(kWaveThreads), fold_smem, s, a, w + L.ct, w + L.cT, w + L.Cfe, w + L.zer);
    if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    // 2. adjoint solve: c~ per (b, t), f~ = 0 (shared), explicit final cost (C_fin, g_T), x~0 = 0; V and v~ are kept
    int rc;
    if (box) {                       // on the masked model; then the forward-value sweep on it, backward only: (f^, c^),
                                     // the true final cost; only v^m is kept
        int32_t *st2 = reinterpret_cast<int32_t *>(w + XL.st2);
        rc = tvlqr_solve_masked_f64(B, n, m, T, c.F, c.sF_b, c.sF_t, w + L.zer, 0, 0, c.C, c.sC_b, c.sC_t, w + L.ct, (long)T * d, d,
                                    a.Cf, a.sCf_b, w + L.cT, n, w + L.zer, w + L.dS, w + L.dA, w + L.dcost, w + L.V, w + L.vt,
                                    c.status, bx.mask, w + L.solve, L.solve_bytes, c.stream);
        if (rc != TFMPC_OK) return rc;
        rc = tvlqr_solve_masked_f64(B, n, m, T, c.F, c.sF_b, c.sF_t, bx.fhat, (long)T * n, n, c.C, c.sC_b, c.sC_t, bx.chat,
                                    (long)T * d, d, a.Cf, a.sCf_b, a.cf, a.scf_b, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    w + XL.vm, st2, bx.mask, w + L.solve, L.solve_bytes, c.stream);
        if (rc != TFMPC_OK) return rc;
        hipLaunchKernelGGL(box_status_or_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, c.status, st2, B);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    } else {
        rc = tfmpc_tvlqr_solve_f64(B, n, m, T, c.F, c.sF_b, c.sF_t, w + L.zer, 0, 0, c.C, c.sC_b, c.sC_t, w + L.ct, (long)T * d, d,
                                   a.Cf, a.sCf_b, w + L.cT, n, w + L.zer, w + L.dS, w + L.dA, w + L.dcost, nullptr, nullptr,
                                   w + L.V, w + L.vt, nullptr, c.status, w + L.solve, L.solve_bytes, c.stream);
        if (rc != TFMPC_OK) return rc;
    }
    // 3. costates and the gradients with a batch stride; batch-shared bounds leave a record per (b, t)
    const bool reduce_F = wants_records(c);
    unsigned per_step = 0, in_time = 0;
    model_wants(a, per_step, in_time);
    const Out bo[2] = {bx.olo, bx.ohi};              // (plain: both NULL)
    for (int k = 0; k < 2; ++k) {
        if (!bo[k].p) continue;
        if (!bo[k].sb) per_step |= 1u << (kRecLo + k);
        else if (bo[k].st == 0 && T > 1) in_time |= 1u << (kLo + k);
        else per_step |= 1u << (kLo + k);
    }
    rc = box ? launch_costates<true>(a, per_step, in_time, reduce_F, bx, s)
             : launch_costates<false>(a, per_step, in_time, reduce_F, {}, s);
    if (rc != TFMPC_OK) return rc;
    // 4. shared gradients: the model's, then the bounds' records
    if ((rc = vjp_shared_sums<double>(a, w + L.partial, s)) != TFMPC_OK) return rc;
    return box ? box_shared_sums<double>(bx, B, T, m, w + L.partial, s) : TFMPC_OK;
}

}  // namespace

namespace tfmpc {

int tvlqr_vjp_f64_fold_launch(const VjpCall<double> &c, double *w, const VjpPrefix &L)
{
    const VjpArgs a = make_args(c, w, L, nullptr, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(vjp_fold_kernel, dim3((unsigned)((size_t)c.B * (c.T + 1))), dim3(kWaveThreads),
                       fold_smem_elems(c.n, c.m) * sizeof(double), static_cast<hipStream_t>(c.stream), a, w + L.ct, w + L.cT,
                       w + L.Cfe, w + L.zer);
    return hipGetLastError() == hipSuccess ? TFMPC_OK : TFMPC_ERR_LAUNCH;
}

int tvlqr_vjp_f64_costates_launch(const VjpCall<double> &c, double *w, const VjpPrefix &L, const double *v, const double *V,
                                  const double *vt, double *P, double *partial)
{
    const VjpArgs a = make_args(c, w, L, v, V, vt, P);
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    unsigned per_step = 0, in_time = 0;
    model_wants(a, per_step, in_time);
    if (const int rc = launch_costates<false>(a, per_step, in_time, wants_records(c), {}, s); rc != TFMPC_OK) return rc;
    return vjp_shared_sums<double>(a, partial, s);
}

}  // namespace tfmpc

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
    return vjp_f64_impl({B, n, m, T, F, sF_b, sF_t, f, sf_b, sf_t, C, sC_b, sC_t, c, sc_b, sc_t, Cfin, sCfin_b, cfin, scfin_b,
                         states, actions, g_states, g_actions, g_costs, dF, sdF_b, sdF_t, df, sdf_b, sdf_t, dC, sdC_b, sdC_t, dc,
                         sdc_b, sdc_t, dCfin, sdCfin_b, dcfin, sdcfin_b, dx0, sdx0_b, status, workspace, workspace_bytes, stream},
                        v, nullptr);
}

size_t tfmpc_tvlqr_box_vjp_workspace_bytes_f64(int B, int n, int m, int T)
{
    if (B <= 0 || n <= 0 || m <= 0 || T <= 0) return 0;
    return box_layout(B, n, m, T).total * sizeof(double);
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
    const BoxCall<double> box{low, slow_b, slow_t, high, shigh_b, shigh_t, dlow, sdlow_b, sdlow_t, dhigh, sdhigh_b, sdhigh_t, clamp_mask};
    return vjp_f64_impl({B, n, m, T, F, sF_b, sF_t, f, sf_b, sf_t, C, sC_b, sC_t, c, sc_b, sc_t, Cfin, sCfin_b, cfin, scfin_b,
                         states, actions, g_states, g_actions, g_costs, dF, sdF_b, sdF_t, df, sdf_b, sdf_t, dC, sdC_b, sdC_t, dc,
                         sdc_b, sdc_t, dCfin, sdCfin_b, dcfin, sdcfin_b, dx0, sdx0_b, status, workspace, workspace_bytes, stream},
                        nullptr, &box);
}

}  // extern "C"

