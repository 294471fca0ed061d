// tvlqr_vjp.hip -- gradients of a time-varying LQR solve (tfmpc_tvlqr_vjp_f32, include/tfmpc_hip.h).
//
// Given the forward trajectory z_t = [x_t; u_t] and upstream gradients on states, actions and costs, the
// vector-Jacobian product is four launches on the caller's stream:
//   1. vjp_fold_kernel    g_t = [gx_t; gu_t] + gcost_t (C_t z_t + c_t), g_T likewise with the final cost; also the
//                         adjoint's explicit final cost (a copy of C_{T-1}[:n,:n] for the default) and its zero x0 / f.
//   2. the TV-LQR solve   (tfmpc_tvlqr_solve_f32, unchanged) with c~_t = g_t, c~_fin = g_T, f~ = 0, x~0 = 0 -> dz_t.
//   3. vjp_sweep_kernel   one wavefront per instance, backward in time (F_t, C_t staged in LDS per step), carrying the costates
//                         lam_t = (C_t z_t + c_t)[:n] + F_t[:, :n]^T lam_{t+1} and dlam_t (the same with dz_t, g_t); it
//                         writes every gradient whose batch stride is non-zero (dF_t = dlam_{t+1} z_t^T + lam_{t+1} dz_t^T,
//                         df_t = dlam_{t+1}, dC_t = (dz z^T + z dz^T + gcost z z^T) / 2, dc_t = dz_t + gcost_t z_t,
//                         dx0 = dlam_0) -- a time stride of 0 accumulates in the output in time order -- and, for
//                         gradients shared by the batch, stores (dlam_{t+1}, lam_{t+1}) per (b, t).
//   4. vjp_reduce_*       gradients with batch stride 0.  dF, df, dC, dc: ONE pass per (chunk of instances, step) emits
//                         all four partial sums -- GEMMs over instances on v_mfma_f32_16x16x4_f32 for n <= 16, d <= 32
//                         (vjp_reduce_steps_mfma16), LDS-tiled scalar sums otherwise (vjp_reduce_steps) -- then a
//                         fixed-order sum over chunks per output (vjp_reduce_steps_stage2).  dCfin, dcfin, dx0: one
//                         record per instance, vjp_reduce_stage1, then the chunks in order (batch_sum.h).  No atomics: the
//                         same call gives the same bits.
// An instance whose adjoint solve reports TFMPC_ST_NOT_PD or TFMPC_ST_SINGULAR contributes NaN (its own rows, and
// any reduction that includes it).  fp32 throughout; no scratch memory.
//
// tfmpc_tvlqr_box_vjp_f32 is the same VJP at a CONTROL-LIMITED optimum: a control that sits on a bound
// (its bits equal low's or high's) is held, du = 0, in the adjoint.  box_fold_kernel also writes the held-set word per
// (b, t) and zeroes the held entries of c~; the adjoint solve is the masked sweep (tvlqr_solve_masked_f32: the mask is
// applied as the model is loaded, no masked copy exists); box_sweep_kernel runs the costate sweep on the UNMASKED model
// and emits r_t[n + i] = (C_t dz_t + g_t + F_t^T dlam_{t+1})[n + i] of every held control into dlow or dhigh;
// box_reduce_bounds sums them over the batch in a fixed order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "batch_sum.h"
#include "lqr_kernels.h"
#include "tvlqr_kernels.h"

using namespace tfmpc;

namespace {

constexpr int kChunk = 256;          // instances per stage-1 partial sum
constexpr int kTile = 16;            // records per LDS tile in stage 1
constexpr int kRedThreads = 256;
constexpr int kEpt = 4;              // output elements per thread per pass in stage 1
constexpr int kSweepThreads = 64;    // one wavefront per instance

enum Kind { kF = 0, kf, kC, kc, kCfin, kcfin, kx0, kKinds };

struct Out {
    float *p;
    long sb, st;
};

struct VjpArgs {
    int B, n, m, T;
    const float *F, *C, *c;
    long sF_b, sF_t, sC_b, sC_t, sc_b, sc_t;
    const float *Cf, *cf;            // final cost as the adjoint sees it (explicit, or the default copy); row stride n
    long sCf_b, scf_b;
    bool dflt;                       // default final cost: its gradients go into dC_{T-1}[:n,:n], dc_{T-1}[:n]
    const float *states, *actions, *gx, *gu, *gc;
    const float *dS, *dA, *ct, *cT;  // adjoint trajectory, c~, c~_fin
    const int32_t *status;
    float *P, *Pf;                   // per (b, t): (dlam_{t+1}, lam_{t+1}) [2n]; per b: dlam_0 [n]
    Out o[kKinds];
};

// The control-limited VJP's extra operands.  R_lo doubles as the fold's record of the unmasked g_u (read by the sweep
// before it overwrites the entry with the bound's gradient).
struct BoxArgs {
    const float *low, *high;
    long slo_b, slo_t, shi_b, shi_t;
    uint32_t *mask, *mask_out;       // [B][T]: workspace, caller's (optional)
    float *Rlo, *Rhi;                // [B][T][m]
    Out olo, ohi;
};

__device__ inline bool same_bits(float x, float y) { return __float_as_uint(x) == __float_as_uint(y); }

__device__ inline float poison_of(const int32_t *status, int b)
{
    return (status[b] & (TFMPC_ST_NOT_PD | TFMPC_ST_SINGULAR)) ? __builtin_nanf("") : 0.0f;
}

// ---- 1. fold -------------------------------------------------------------------------------------------------------
// One wavefront per (b, t); t == T is the final step (rows < n).  With a cost gradient, C_t is staged in LDS by
// coalesced loads (row stride d + 1) and each lane takes rows of C_t z_t + c_t.
template <bool BOX>
__device__ __forceinline__ void fold_body(const VjpArgs &a, float *ct, float *cT, float *Cfe, float *zer, const float *c_op,
                                          long sc_b, long sc_t, const float *Cfin_user, const BoxArgs *bx)
{
    extern __shared__ float sm[];
    const int n = a.n, m = a.m, T = a.T, d = n + m, L = threadIdx.x;
    const int b = (int)(blockIdx.x / (T + 1)), t = (int)(blockIdx.x % (T + 1));
    const float *x = a.states + ((size_t)b * (T + 1) + t) * n;
    if (t < T) {
        uint32_t held = 0;
        if (BOX) {                   // lane i < m (m <= 32): is control i on a bound, bit for bit?
            bool on = false;
            if (L < m) {
                const float u = a.actions[((size_t)b * T + t) * m + L];
                on = same_bits(u, tv_at(bx->low, bx->slo_b, bx->slo_t, b, t)[L]) ||
                     same_bits(u, tv_at(bx->high, bx->shi_b, bx->shi_t, b, t)[L]);
            }
            held = (uint32_t)__ballot(on);
            if (L == 0) {
                bx->mask[(size_t)b * T + t] = held;
                if (bx->mask_out) bx->mask_out[(size_t)b * T + t] = held;
            }
        }
        float *sC = sm, *sz = sm + (size_t)d * (d + 1);
        if (a.gc) {
            const float *Ct = tv_at(a.C, a.sC_b, a.sC_t, b, t);
            for (int e = L; e < d * d; e += 64) sC[(e / d) * (d + 1) + e % d] = Ct[e];
            const float *u = a.actions + ((size_t)b * T + t) * m;
            for (int i = L; i < d; i += 64) sz[i] = i < n ? x[i] : u[i - n];
            __syncthreads();
        }
        for (int i = L; i < d; i += 64) {
            float g = 0.0f;
            if (i < n) { if (a.gx) g = a.gx[((size_t)b * (T + 1) + t) * n + i]; }
            else if (a.gu) g = a.gu[((size_t)b * T + t) * m + (i - n)];
            if (a.gc) {
                const float w = a.gc[(size_t)b * (T + 1) + t];
                const float *Ci = sC + (size_t)i * (d + 1);
                float r = tv_at(c_op, sc_b, sc_t, b, t)[i];
                for (int j = 0; j < d; ++j) r = fmaf(Ci[j], sz[j], r);
                g = fmaf(w, r, g);
            }
            if (BOX && i >= n) {
                bx->Rlo[((size_t)b * T + t) * m + (i - n)] = g;
                if (held >> (i - n) & 1u) g = 0.0f;
            }
            ct[((size_t)b * T + t) * d + i] = g;
        }
        return;
    }
    for (int i = L; i < n; i += 64) {
        zer[(size_t)b * n + i] = 0.0f;
        const float *Crow;
        float r;
        if (a.dflt) {                // C_{T-1}[i, :n], c_{T-1}[i]: copy the row into the adjoint's explicit final cost
            Crow = tv_at(a.C, a.sC_b, a.sC_t, b, T - 1) + (size_t)i * d;
            r = tv_at(c_op, sc_b, sc_t, b, T - 1)[i];
            if (a.sCf_b != 0 || b == 0)
                for (int j = 0; j < n; ++j) Cfe[(size_t)b * a.sCf_b + (size_t)i * n + j] = Crow[j];
        } else {
            Crow = Cfin_user + (size_t)b * a.sCf_b + (size_t)i * n;
            r = a.cf[(size_t)b * a.scf_b + i];
        }
        float g = a.gx ? a.gx[((size_t)b * (T + 1) + T) * n + i] : 0.0f;
        if (a.gc) {
            for (int j = 0; j < n; ++j) r = fmaf(Crow[j], x[j], r);
            g = fmaf(a.gc[(size_t)b * (T + 1) + T], r, g);
        }
        cT[(size_t)b * n + i] = g;
    }
}

__global__ void __launch_bounds__(64) vjp_fold_kernel(VjpArgs a, float *ct, float *cT, float *Cfe, float *zer,
                                                      const float *c_op, long sc_b, long sc_t, const float *Cfin_user)
{
    fold_body<false>(a, ct, cT, Cfe, zer, c_op, sc_b, sc_t, Cfin_user, nullptr);
}

__global__ void __launch_bounds__(64) box_fold_kernel(VjpArgs a, float *ct, float *cT, float *Cfe, float *zer,
                                                      const float *c_op, long sc_b, long sc_t, const float *Cfin_user,
                                                      BoxArgs bx)
{
    fold_body<true>(a, ct, cT, Cfe, zer, c_op, sc_b, sc_t, Cfin_user, &bx);
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
    const float poison = poison_of(a.status, b);
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
            else a.Pf[(size_t)b * n + i] = dlam[i];
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

// Bound gradients shared by the batch: partial[(chunk * T + t) * m + e] = sum over the chunk's instances of R[b][t][e],
// eight interleaved sub-sums per element combined in a fixed order (m <= 32); box_reduce_final sums the chunks.
__global__ void __launch_bounds__(kRedThreads) box_reduce_bounds(const float *R, int B, int T, int m, float *partial)
{
    __shared__ float sub[kRedThreads];
    const int chunk = blockIdx.x, t = blockIdx.y, e = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int b0 = chunk * kChunk, b1 = min(B, b0 + kChunk);
    float s = 0.0f;
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
// (element, slot), 256 strided sub-sums and an LDS tree -- a fixed order, so the same call gives the same bits.
__global__ void __launch_bounds__(kRedThreads) box_reduce_final(const float *partial, int chunks, int T, int m, bool timed,
                                                                float *out, long st)
{
    __shared__ float sub[kRedThreads];
    const int e = blockIdx.x, slot = blockIdx.y, tid = threadIdx.x;
    const int t0 = timed ? slot : 0, nt = timed ? 1 : T, total = chunks * nt;
    float s = 0.0f;
    for (int q = tid; q < total; q += kRedThreads) s += partial[((size_t)(q / nt) * T + t0 + q % nt) * m + e];
    sub[tid] = s;
    __syncthreads();
    for (int w = kRedThreads / 2; w > 0; w >>= 1) {
        if (tid < w) sub[tid] += sub[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[(size_t)slot * st + e] = sub[0];
}

// ---- 4. batch reductions ---------------------------------------------------------------------------------------------
// A record of instance b: a[n] l[n] z[d] dz[d] gc.  Step records (t < T) take a = dlam_{t+1}, l = lam_{t+1}; the final
// record takes z[:n] = x_T, dz[:n] = dx_T, gc = gcost_T and a = dlam_0.
__device__ inline void load_record(const VjpArgs &a, float *rec, int b, int t, bool fin, int lane, int nthr)
{
    const int n = a.n, m = a.m, T = a.T, d = n + m, W = 2 * n + 2 * d + 1;
    const float poison = poison_of(a.status, b);
    for (int q = lane; q < W; q += nthr) {
        float v;
        if (q < 2 * n) {
            if (fin) v = q < n && a.Pf ? a.Pf[(size_t)b * n + q] : 0.0f;
            else v = a.P ? a.P[((size_t)b * T + t) * 2 * n + q] : 0.0f;
        } else if (q < 2 * n + d) {
            const int i = q - 2 * n;
            if (fin) v = i < n ? a.states[((size_t)b * (T + 1) + T) * n + i] : 0.0f;
            else v = i < n ? a.states[((size_t)b * (T + 1) + t) * n + i] : a.actions[((size_t)b * T + t) * m + i - n];
        } else if (q < 2 * n + 2 * d) {
            const int i = q - 2 * n - d;
            if (fin) v = i < n ? a.dS[((size_t)b * (T + 1) + T) * n + i] : 0.0f;
            else v = i < n ? a.dS[((size_t)b * (T + 1) + t) * n + i] : a.dA[((size_t)b * T + t) * m + i - n];
        } else {
            v = a.gc ? a.gc[(size_t)b * (T + 1) + (fin ? T : t)] : 0.0f;
        }
        rec[q] = v + poison;
    }
}

__device__ inline float contrib(int kind, const float *r, int n, int d, int e, bool fin_into_step)
{
    const float *al = r, *l = r + n, *z = r + 2 * n, *dz = z + d, gc = z[2 * d];
    switch (kind) {
    case kF: { const int i = e / d, j = e % d; return fmaf(al[i], z[j], l[i] * dz[j]); }
    case kf: return al[e];
    case kC: {
        const int i = e / d, j = e % d;
        if (fin_into_step && (i >= n || j >= n)) return 0.0f;
        return 0.5f * (dz[i] * z[j] + z[i] * dz[j] + gc * z[i] * z[j]);
    }
    case kc: if (fin_into_step && e >= n) return 0.0f; return dz[e] + gc * z[e];
    case kCfin: { const int i = e / n, j = e % n; return 0.5f * (dz[i] * z[j] + z[i] * dz[j] + gc * z[i] * z[j]); }
    case kcfin: return dz[e] + gc * z[e];
    default: return al[e];       // kx0
    }
}

// grid (chunks, time slots); partial[(chunk * slots + slot) * nE + e]
__global__ void __launch_bounds__(kRedThreads) vjp_reduce_stage1(VjpArgs a, int kind, int nE, int slots, float *partial)
{
    extern __shared__ float tile[];
    const int n = a.n, d = n + a.m, T = a.T, W = 2 * n + 2 * d + 1;
    const int chunk = blockIdx.x, slot = blockIdx.y, tid = threadIdx.x;
    const int b0 = chunk * kChunk, b1 = min(a.B, b0 + kChunk);
    const bool final_kind = kind == kCfin || kind == kcfin || kind == kx0;
    // time range of this slot; final-record kinds have one (virtual) step
    const int t0 = final_kind ? 0 : (slots == 1 ? 0 : slot), t1 = final_kind ? 1 : (slots == 1 ? T : slot + 1);
    const bool add_final = a.dflt && (kind == kC || kind == kc) && T - 1 >= t0 && T - 1 < t1;
    for (int e0 = 0; e0 < nE; e0 += kRedThreads * kEpt) {
        float acc[kEpt];
        for (int q = 0; q < kEpt; ++q) acc[q] = 0.0f;
        // passes: the steps of the slot in time order, then (default final cost) the final records
        for (int pass = t0; pass < t1 + (add_final ? 1 : 0); ++pass) {
            const bool fin = final_kind || pass == t1;
            for (int bb = b0; bb < b1; bb += kTile) {
                const int nb = min(kTile, b1 - bb);
                __syncthreads();
                for (int r = tid / 16; r < nb; r += kRedThreads / 16)
                    load_record(a, tile + r * W, bb + r, pass, fin, tid % 16, 16);
                __syncthreads();
                for (int r = 0; r < nb; ++r)
                    for (int q = 0; q < kEpt; ++q) {
                        const int e = e0 + q * kRedThreads + tid;
                        if (e < nE) acc[q] += contrib(kind, tile + r * W, n, d, e, fin && !final_kind);
                    }
            }
        }
        for (int q = 0; q < kEpt; ++q) {
            const int e = e0 + q * kRedThreads + tid;
            if (e < nE) partial[((size_t)chunk * slots + slot) * nE + e] = acc[q];
        }
    }
}

// Fused per-step reductions: ONE pass over the records emits every requested batch-shared per-step gradient (dF, df,
// dC, dc) of a chunk of instances at step t.  partial[(chunk * T + t) * E + off_k + e], E = n d + n + d d + d.
__host__ __device__ inline int steps_E(int n, int d) { return n * d + n + d * d + d; }
__host__ __device__ inline int steps_off(int k, int n, int d)
{
    return k == kF ? 0 : k == kf ? n * d : k == kC ? n * d + n : n * d + n + d * d;
}

// Shape-generic form: records staged in LDS tiles, scalar sums over the concatenated outputs.
__global__ void __launch_bounds__(kRedThreads) vjp_reduce_steps(VjpArgs a, unsigned need, float *partial)
{
    extern __shared__ float tile[];
    const int n = a.n, d = n + a.m, T = a.T, W = 2 * n + 2 * d + 1, E = steps_E(n, d);
    const int chunk = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int b0 = chunk * kChunk, b1 = min(a.B, b0 + kChunk);
    const int passes = (a.dflt && t == T - 1) ? 2 : 1;      // pass 1: the default final cost's records into dC, dc
    for (int e0 = 0; e0 < E; e0 += kRedThreads * kEpt) {
        float acc[kEpt];
        int kind[kEpt], ee[kEpt];
        for (int q = 0; q < kEpt; ++q) {
            acc[q] = 0.0f;
            const int e = e0 + q * kRedThreads + tid;
            kind[q] = e < steps_off(kf, n, d) ? kF : e < steps_off(kC, n, d) ? kf : e < steps_off(kc, n, d) ? kC : kc;
            ee[q] = e - steps_off(kind[q], n, d);
        }
        for (int pass = 0; pass < passes; ++pass) {
            const bool fin = pass == 1;
            for (int bb = b0; bb < b1; bb += kTile) {
                const int nb = min(kTile, b1 - bb);
                __syncthreads();
                for (int r = tid / 16; r < nb; r += kRedThreads / 16)
                    load_record(a, tile + r * W, bb + r, t, fin, tid % 16, 16);
                __syncthreads();
                for (int r = 0; r < nb; ++r)
                    for (int q = 0; q < kEpt; ++q) {
                        const int e = e0 + q * kRedThreads + tid;
                        if (e >= E || !(need >> kind[q] & 1u) || (fin && kind[q] <= kf)) continue;
                        acc[q] += contrib(kind[q], tile + r * W, n, d, ee[q], fin);
                    }
            }
        }
        for (int q = 0; q < kEpt; ++q) {
            const int e = e0 + q * kRedThreads + tid;
            if (e < E) partial[((size_t)chunk * T + t) * E + e] = acc[q];
        }
    }
}

// n <= 16, d <= 32: the batch sums are GEMMs over instances on v_mfma_f32_16x16x4_f32 (fp32 operands and
// accumulation), four instances per k-step, one wave per (chunk, t).  Lane (li = lane & 15, lq = lane >> 4) loads
// instance b0 + lq's entries li and 16 + li straight into the A / B operand slots:
//   dF = [dlam | lam] [z | dz]^T            (two 16 x 16 column tiles)
//   dC = ([dz | z] [z | dz + gc z]^T) / 2   (2 x 2 tiles)
// df and dc are per-lane sums, combined over the four k-groups in a fixed order.
__global__ void __launch_bounds__(64) vjp_reduce_steps_mfma16(VjpArgs a, unsigned need, float *partial)
{
    using f32x4 = __attribute__((ext_vector_type(4))) float;
    const int n = a.n, m = a.m, T = a.T, d = n + m, E = steps_E(n, d);
    const int chunk = blockIdx.x, t = blockIdx.y, lane = threadIdx.x, li = lane & 15, lq = lane >> 4;
    const int b0 = chunk * kChunk, b1 = min(a.B, b0 + kChunk);
    const bool wantF = need & ((1u << kF) | (1u << kf)), wantC = need & ((1u << kC) | (1u << kc));
    f32x4 F0 = {0, 0, 0, 0}, F1 = F0, C00 = F0, C01 = F0, C10 = F0, C11 = F0;
    float sf = 0.0f, sc0 = 0.0f, sc1 = 0.0f;
    const int passes = (a.dflt && t == T - 1) ? 2 : 1;
    for (int pass = 0; pass < passes; ++pass) {
        const bool fin = pass == 1;
        const int ts = fin ? T : t;
        for (int bb = b0; bb < b1; bb += 4) {
            const int b = bb + lq;
            float av = 0.0f, lv = 0.0f, z0 = 0.0f, z1 = 0.0f, dz0 = 0.0f, dz1 = 0.0f, gc = 0.0f;
            if (b < b1) {
                const float p = poison_of(a.status, b);
                const float *x = a.states + ((size_t)b * (T + 1) + ts) * n, *dx = a.dS + ((size_t)b * (T + 1) + ts) * n;
                const float *u = a.actions + ((size_t)b * T + t) * m, *du = a.dA + ((size_t)b * T + t) * m;
                const int j1 = 16 + li;
                if (fin) {
                    if (li < n) { z0 = x[li]; dz0 = dx[li]; }
                } else {
                    if (wantF && li < n) {
                        const float *P = a.P + ((size_t)b * T + t) * 2 * n;
                        av = P[li] + p;
                        lv = P[n + li] + p;
                    }
                    if (li < d) { z0 = li < n ? x[li] : u[li - n]; dz0 = li < n ? dx[li] : du[li - n]; }
                    if (j1 < d) { z1 = j1 < n ? x[j1] : u[j1 - n]; dz1 = j1 < n ? dx[j1] : du[j1 - n]; }
                }
                z0 += p; z1 += p; dz0 += p; dz1 += p;
                if (a.gc) gc = a.gc[(size_t)b * (T + 1) + ts];
                gc += p;
            }
            const float w0 = fmaf(gc, z0, dz0), w1 = fmaf(gc, z1, dz1);
            if (wantF && !fin) {
                F0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, z0, F0, 0, 0, 0);
                F0 = __builtin_amdgcn_mfma_f32_16x16x4f32(lv, dz0, F0, 0, 0, 0);
                F1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, z1, F1, 0, 0, 0);
                F1 = __builtin_amdgcn_mfma_f32_16x16x4f32(lv, dz1, F1, 0, 0, 0);
                sf += av;
            }
            if (wantC) {
                C00 = __builtin_amdgcn_mfma_f32_16x16x4f32(dz0, z0, C00, 0, 0, 0);
                C00 = __builtin_amdgcn_mfma_f32_16x16x4f32(z0, w0, C00, 0, 0, 0);
                C01 = __builtin_amdgcn_mfma_f32_16x16x4f32(dz0, z1, C01, 0, 0, 0);
                C01 = __builtin_amdgcn_mfma_f32_16x16x4f32(z0, w1, C01, 0, 0, 0);
                C10 = __builtin_amdgcn_mfma_f32_16x16x4f32(dz1, z0, C10, 0, 0, 0);
                C10 = __builtin_amdgcn_mfma_f32_16x16x4f32(z1, w0, C10, 0, 0, 0);
                C11 = __builtin_amdgcn_mfma_f32_16x16x4f32(dz1, z1, C11, 0, 0, 0);
                C11 = __builtin_amdgcn_mfma_f32_16x16x4f32(z1, w1, C11, 0, 0, 0);
                sc0 += w0;
                sc1 += w1;
            }
        }
    }
    float *out = partial + ((size_t)chunk * T + t) * E;
    // the four k-groups of lane li, summed in a fixed order
    auto fold4 = [&](float v) {
        return ((__shfl(v, li) + __shfl(v, li + 16)) + __shfl(v, li + 32)) + __shfl(v, li + 48);
    };
    const float tf = fold4(sf), tc0 = fold4(sc0), tc1 = fold4(sc1);
    for (int r = 0; r < 4; ++r) {
        const int i = 4 * lq + r;
        if (i < n) {
            if (li < d) out[i * d + li] = F0[r];
            if (16 + li < d) out[i * d + 16 + li] = F1[r];
        }
        const int cb = steps_off(kC, n, d);
        if (i < d && li < d) out[cb + i * d + li] = 0.5f * C00[r];
        if (i < d && 16 + li < d) out[cb + i * d + 16 + li] = 0.5f * C01[r];
        if (16 + i < d && li < d) out[cb + (16 + i) * d + li] = 0.5f * C10[r];
        if (16 + i < d && 16 + li < d) out[cb + (16 + i) * d + 16 + li] = 0.5f * C11[r];
    }
    if (lq == 0) {
        if (li < n) out[steps_off(kf, n, d) + li] = tf;
        if (li < d) out[steps_off(kc, n, d) + li] = tc0;
        if (16 + li < d) out[steps_off(kc, n, d) + 16 + li] = tc1;
    }
}

// Stage 2 of the per-step outputs: out[slot * st + e] = sum over chunks, then over the slot's steps, in that order.
__global__ void vjp_reduce_steps_stage2(const float *partial, int chunks, int T, int E, int off, int nE, bool timed,
                                        float *out, long st)
{
    const int slots = timed ? T : 1;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)slots * nE) return;
    const int slot = (int)(idx / nE), e = (int)(idx % nE);
    const int t0 = timed ? slot : 0, t1 = timed ? slot + 1 : T;
    float s = 0.0f;
    for (int k = 0; k < chunks; ++k)
        for (int t = t0; t < t1; ++t) s += partial[((size_t)k * T + t) * E + off + e];
    out[(size_t)slot * st + e] = s;
}

// ---- launch helpers --------------------------------------------------------------------------------------------------
size_t fold_smem_bytes(int n, int m) { const size_t d = n + m; return (d * (d + 1) + d) * sizeof(float); }

size_t sweep_smem_bytes(int n, int m)
{
    const size_t d = n + m;
    return (3 * d + 6 * (size_t)n + (size_t)n * d + d * (d + 1)) * sizeof(float);
}

template <typename K>
bool allow_lds(K kern, size_t smem)
{
    return smem <= 64 * 1024 || hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) == hipSuccess;
}

// ---- workspace -------------------------------------------------------------------------------------------------------
struct Layout {
    size_t ct, cT, Cfe, zer, dS, dA, dcost, solve, P, Pf, partial, total;   // offsets in floats
    size_t solve_bytes;
};

size_t up64(size_t x) { return (x + 63) / 64 * 64; }

Layout layout(int B, int n, int m, int T)
{
    const size_t d = n + m, Bs = B, Ts = T, chunks = (Bs + kChunk - 1) / kChunk;
    Layout L{};
    size_t o = 0;
    L.ct = o; o += up64(Bs * Ts * d);
    L.cT = o; o += up64(Bs * n);
    L.Cfe = o; o += up64(Bs * n * n);
    L.zer = o; o += up64(Bs * n);
    L.dS = o; o += up64(Bs * (Ts + 1) * n);
    L.dA = o; o += up64(Bs * Ts * m);
    L.dcost = o; o += up64(Bs * (Ts + 1));
    L.solve_bytes = tfmpc_tvlqr_workspace_bytes(B, n, m, T);
    L.solve = o; o += up64((L.solve_bytes + 3) / 4);
    L.P = o; o += up64(Bs * Ts * 2 * n);
    L.Pf = o; o += up64(Bs * n);
    L.partial = o; o += up64(chunks * Ts * (size_t)steps_E(n, (int)d));   // >= chunks * n * n of the final-cost sums
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

struct BoxCall {
    const float *low, *high;
    long slo_b, slo_t, shi_b, shi_t;
    float *dlow, *dhigh;
    long sdlo_b, sdlo_t, sdhi_b, sdhi_t;
    uint32_t *clamp_mask;
};

int vjp_impl(int B, int n, int m, int T,
             const float *F, long sF_b, long sF_t, const float *f, long sf_b, long sf_t,
             const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t,
             const float *Cfin, long sCfin_b, const float *cfin, long scfin_b,
             const float *states, const float *actions,
             const float *g_states, const float *g_actions, const float *g_costs,
             float *dF, long sdF_b, long sdF_t, float *df, long sdf_b, long sdf_t,
             float *dC, long sdC_b, long sdC_t, float *dc, long sdc_b, long sdc_t,
             float *dCfin, long sdCfin_b, float *dcfin, long sdcfin_b, float *dx0, long sdx0_b,
             int32_t *status, void *workspace, size_t workspace_bytes, void *stream, const BoxCall *box);

}  // namespace

extern "C" {

size_t tfmpc_tvlqr_vjp_workspace_bytes(int B, int n, int m, int T)
{
    if (B <= 0 || n <= 0 || m <= 0 || T <= 0) return 0;
    return layout(B, n, m, T).total * sizeof(float);
}

#define TFMPC_VJP_PARAMS_HEAD                                                                                      \
    int B, int n, int m, int T, const float *F, long sF_b, long sF_t, const float *f, long sf_b, long sf_t,          \
        const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t, const float *Cfin, long sCfin_b, \
        const float *cfin, long scfin_b
#define TFMPC_VJP_PARAMS_TAIL                                                                                      \
    const float *states, const float *actions, const float *g_states, const float *g_actions, const float *g_costs, \
        float *dF, long sdF_b, long sdF_t, float *df, long sdf_b, long sdf_t, float *dC, long sdC_b, long sdC_t,    \
        float *dc, long sdc_b, long sdc_t, float *dCfin, long sdCfin_b, float *dcfin, long sdcfin_b, float *dx0,    \
        long sdx0_b
#define TFMPC_VJP_HEAD B, n, m, T, F, sF_b, sF_t, f, sf_b, sf_t, C, sC_b, sC_t, c, sc_b, sc_t, Cfin, sCfin_b, cfin, scfin_b
#define TFMPC_VJP_TAIL                                                                                             \
    states, actions, g_states, g_actions, g_costs, dF, sdF_b, sdF_t, df, sdf_b, sdf_t, dC, sdC_b, sdC_t, dc, sdc_b, \
        sdc_t, dCfin, sdCfin_b, dcfin, sdcfin_b, dx0, sdx0_b

int tfmpc_tvlqr_vjp_f32(TFMPC_VJP_PARAMS_HEAD, TFMPC_VJP_PARAMS_TAIL, int32_t *status, void *workspace,
                        size_t workspace_bytes, void *stream)
{
    return vjp_impl(TFMPC_VJP_HEAD, TFMPC_VJP_TAIL, status, workspace, workspace_bytes, stream, nullptr);
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

int tfmpc_tvlqr_box_vjp_f32(TFMPC_VJP_PARAMS_HEAD, const float *low, long slow_b, long slow_t, const float *high,
                            long shigh_b, long shigh_t, TFMPC_VJP_PARAMS_TAIL, float *dlow, long sdlow_b, long sdlow_t,
                            float *dhigh, long sdhigh_b, long sdhigh_t, uint32_t *clamp_mask, int32_t *status,
                            void *workspace, size_t workspace_bytes, void *stream)
{
    const BoxCall box{low, high, slow_b, slow_t, shigh_b, shigh_t, dlow, dhigh, sdlow_b, sdlow_t, sdhigh_b, sdhigh_t,
                      clamp_mask};
    return vjp_impl(TFMPC_VJP_HEAD, TFMPC_VJP_TAIL, status, workspace, workspace_bytes, stream, &box);
}

}  // extern "C"

namespace {

int vjp_impl(TFMPC_VJP_PARAMS_HEAD, TFMPC_VJP_PARAMS_TAIL, int32_t *status, void *workspace, size_t workspace_bytes,
             void *stream, const BoxCall *box)
{
    if (B < 0 || n <= 0 || m <= 0 || T <= 0) return TFMPC_ERR_ARG;
    if (!tvlqr_mfma_supported(n, m) && tvlqr_generic_smem_bytes(n, m) > kMaxLdsBytes) return TFMPC_ERR_UNSUPPORTED;
    if (B == 0) return TFMPC_OK;
    if (!F || !f || !C || !c || !states || !actions || !status) return TFMPC_ERR_ARG;
    if (!Cfin != !cfin) return TFMPC_ERR_ARG;
    if (!Cfin && (dCfin || dcfin)) return TFMPC_ERR_ARG;           // the default final cost's gradient is in dC, dc
    if (T > 65535) return TFMPC_ERR_UNSUPPORTED;                   // per-step reduction slots are one grid axis
    if ((size_t)B * (T + 1) > 0x7fffffffu) return TFMPC_ERR_UNSUPPORTED;   // fold: one block per (b, t)
    if (sweep_smem_bytes(n, m) > kMaxLdsBytes || fold_smem_bytes(n, m) > kMaxLdsBytes) return TFMPC_ERR_UNSUPPORTED;
    if (box) {
        if (m > 32) return TFMPC_ERR_UNSUPPORTED;                  // one held-set word per step
        if (!box->low || !box->high) return TFMPC_ERR_ARG;
        for (long s : {box->slo_b, box->slo_t, box->shi_b, box->shi_t, box->sdlo_b, box->sdlo_t, box->sdhi_b, box->sdhi_t})
            if (s < 0) return TFMPC_ERR_ARG;
    }
    for (long s : {sF_b, sF_t, sf_b, sf_t, sC_b, sC_t, sc_b, sc_t, sCfin_b, scfin_b, sdF_b, sdF_t, sdf_b, sdf_t,
                   sdC_b, sdC_t, sdc_b, sdc_t, sdCfin_b, sdcfin_b, sdx0_b})
        if (s < 0) return TFMPC_ERR_ARG;
    const Layout L = layout(B, n, m, T);
    const BoxLayout XL = box ? box_layout(B, n, m, T) : BoxLayout{};
    if (!workspace || workspace_bytes < (box ? XL.total : L.total) * sizeof(float)) return TFMPC_ERR_WORKSPACE;
    const int d = n + m;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *w = static_cast<float *>(workspace);

    VjpArgs a{};
    a.B = B; a.n = n; a.m = m; a.T = T;
    a.F = F; a.sF_b = sF_b; a.sF_t = sF_t;
    a.C = C; a.sC_b = sC_b; a.sC_t = sC_t;
    a.c = c; a.sc_b = sc_b; a.sc_t = sc_t;
    a.dflt = Cfin == nullptr;
    a.states = states; a.actions = actions; a.gx = g_states; a.gu = g_actions; a.gc = g_costs;
    a.dS = w + L.dS; a.dA = w + L.dA; a.ct = w + L.ct; a.cT = w + L.cT;
    a.status = status;
    a.P = w + L.P; a.Pf = w + L.Pf;
    if (a.dflt) {
        a.Cf = w + L.Cfe; a.sCf_b = sC_b ? (long)n * n : 0;
        a.cf = nullptr; a.scf_b = 0;
    } else {
        a.Cf = Cfin; a.sCf_b = sCfin_b;
        a.cf = cfin; a.scf_b = scfin_b;
    }
    Out outs[kKinds] = {{dF, sdF_b, sdF_t}, {df, sdf_b, sdf_t}, {dC, sdC_b, sdC_t}, {dc, sdc_b, sdc_t},
                        {dCfin, sdCfin_b, 0}, {dcfin, sdcfin_b, 0}, {dx0, sdx0_b, 0}};
    for (int k = 0; k < kKinds; ++k) a.o[k] = outs[k];
    BoxArgs bx{};
    if (box) {
        bx.low = box->low; bx.slo_b = box->slo_b; bx.slo_t = box->slo_t;
        bx.high = box->high; bx.shi_b = box->shi_b; bx.shi_t = box->shi_t;
        bx.mask = reinterpret_cast<uint32_t *>(w + XL.mask); bx.mask_out = box->clamp_mask;
        bx.Rlo = w + XL.Rlo; bx.Rhi = w + XL.Rhi;
        bx.olo = Out{box->dlow, box->sdlo_b, box->sdlo_t};
        bx.ohi = Out{box->dhigh, box->sdhi_b, box->sdhi_t};
    }

    // 1. fold
    {
        const size_t smem = fold_smem_bytes(n, m);
        const dim3 grid((unsigned)((size_t)B * (T + 1)));
        if (box) {
            if (!allow_lds(box_fold_kernel, smem)) return TFMPC_ERR_LAUNCH;
            hipLaunchKernelGGL(box_fold_kernel, grid, dim3(64), smem, s, a, w + L.ct, w + L.cT, w + L.Cfe, w + L.zer, c, sc_b,
                               sc_t, Cfin, bx);
        } else {
            if (!allow_lds(vjp_fold_kernel, smem)) return TFMPC_ERR_LAUNCH;
            hipLaunchKernelGGL(vjp_fold_kernel, grid, dim3(64), smem, s, a, w + L.ct, w + L.cT, w + L.Cfe, w + L.zer, c, sc_b,
                               sc_t, Cfin);
        }
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    // 2. adjoint solve: c~ per (b, t), f~ = 0 (shared), explicit final cost, x~0 = 0
    {
        const float *Cf_adj = a.dflt ? w + L.Cfe : Cfin;
        const long sCf_adj = a.dflt ? a.sCf_b : sCfin_b;
        int rc;
        if (box)                     // the held controls taken out of the model as it is loaded
            rc = tvlqr_solve_masked_f32(B, n, m, T, F, sF_b, sF_t, w + L.zer, 0, 0, C, sC_b, sC_t, w + L.ct, (long)T * d, d,
                                        Cf_adj, sCf_adj, w + L.cT, n, w + L.zer, w + L.dS, w + L.dA, w + L.dcost, status,
                                        bx.mask, w + L.solve, L.solve_bytes, stream);
        else
            rc = tfmpc_tvlqr_solve_f32(B, n, m, T, F, sF_b, sF_t, w + L.zer, 0, 0, C, sC_b, sC_t, w + L.ct, (long)T * d, d,
                                       Cf_adj, sCf_adj, w + L.cT, n, w + L.zer, w + L.dS, w + L.dA, w + L.dcost, nullptr,
                                       nullptr, nullptr, nullptr, nullptr, status, w + L.solve, L.solve_bytes, stream);
        if (rc != TFMPC_OK) return rc;
    }
    // for the sweep, the final cost's linear term is the forward's: default c_{T-1}[:n] (contiguous in c at stride 1)
    VjpArgs sw = a;
    if (a.dflt) {
        sw.cf = c + (size_t)(T - 1) * sc_t; sw.scf_b = sc_b;
    }
    // 3. sweep
    const bool reduce_F = (dF && !sdF_b) || (df && !sdf_b);
    {
        const size_t smem = sweep_smem_bytes(n, m);
        if (box) {
            if (!allow_lds(box_sweep_kernel, smem)) return TFMPC_ERR_LAUNCH;
            hipLaunchKernelGGL(box_sweep_kernel, dim3(B), dim3(kSweepThreads), smem, s, sw, reduce_F, bx);
        } else {
            if (!allow_lds(vjp_sweep_kernel, smem)) return TFMPC_ERR_LAUNCH;
            hipLaunchKernelGGL(vjp_sweep_kernel, dim3(B), dim3(kSweepThreads), smem, s, sw, reduce_F);
        }
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    // 4. shared gradients
    const int chunks = (B + kChunk - 1) / kChunk;
    const int W = 2 * n + 2 * d + 1;
    const int nEs[kKinds] = {n * d, n, d * d, d, n * n, n, n};
    float *partial = w + L.partial;
    unsigned need = 0;
    for (int k = kF; k <= kc; ++k)
        if (a.o[k].p && !a.o[k].sb) need |= 1u << k;
    if (need) {                      // dF, df, dC, dc: one pass over the records, then one short sum per output
        if (n <= 16 && d <= 32)
            hipLaunchKernelGGL(vjp_reduce_steps_mfma16, dim3(chunks, T), dim3(64), 0, s, sw, need, partial);
        else
            hipLaunchKernelGGL(vjp_reduce_steps, dim3(chunks, T), dim3(kRedThreads), (size_t)kTile * W * sizeof(float), s,
                               sw, need, partial);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
        for (int k = kF; k <= kc; ++k) {
            if (!(need >> k & 1u)) continue;
            const bool timed = a.o[k].st != 0;
            const size_t total = (size_t)(timed ? T : 1) * nEs[k];
            hipLaunchKernelGGL(vjp_reduce_steps_stage2, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, partial,
                               chunks, T, steps_E(n, d), steps_off(k, n, d), nEs[k], timed, a.o[k].p, a.o[k].st);
            if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
        }
    }
    for (int k = kCfin; k < kKinds; ++k) {      // final-cost and x0 sums: one record per instance
        const Out &o = a.o[k];
        if (!o.p || o.sb) continue;
        hipLaunchKernelGGL(vjp_reduce_stage1, dim3(chunks, 1), dim3(kRedThreads), (size_t)kTile * W * sizeof(float), s,
                           sw, k, nEs[k], 1, partial);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
        hipLaunchKernelGGL(batch_sum_stage2_in_order<kRedThreads>, dim3((unsigned)((nEs[k] + 255) / 256)), dim3(kRedThreads), 0, s,
                           partial, chunks, (size_t)nEs[k], nEs[k], o.p, 0L);      // the chunks in order (batch_sum.h)
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    if (box) {                       // bound gradients shared by the batch: the sweep's records, chunks, then steps
        const Out bo[2] = {bx.olo, bx.ohi};
        const float *rec[2] = {bx.Rlo, bx.Rhi};
        for (int k = 0; k < 2; ++k) {
            if (!bo[k].p || bo[k].sb) continue;
            hipLaunchKernelGGL(box_reduce_bounds, dim3(chunks, T), dim3(kRedThreads), 0, s, rec[k], B, T, m, partial);
            if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
            const bool timed = bo[k].st != 0;
            hipLaunchKernelGGL(box_reduce_final, dim3(m, timed ? T : 1), dim3(kRedThreads), 0, s, partial, chunks, T, m, timed,
                               bo[k].p, bo[k].st);
            if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
        }
    }
    return TFMPC_OK;
}

}  // namespace
