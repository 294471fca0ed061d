// tvlqr_vjp_common.h -- what the gradients of the fp32 and of the double-precision TV-LQR solve share (tvlqr_vjp.hip,
// tvlqr_vjp_f64.hip), templated on the scalar S: the fold, the batch reductions (the
// model's and the bounds') with the host code that enqueues them, and the argument contract of the four C entries --
// their arguments as one aggregate, the checks that do not depend on a precision's kernels, the fill of VjpBase<S>.
// The two files differ in the costates (open-loop recursion / value function), which stay there.
//
// Batch reductions: gradients with batch stride 0.  dF, df, dC, dc: ONE pass per (chunk of instances, step) emits all
// four partial sums -- GEMMs over instances on the 16x16x4 matrix-core instruction of S for n <= 16, d <= 32
// (vjp_reduce_steps_mfma16), LDS-tiled scalar sums otherwise (vjp_reduce_steps) -- then a fixed-order sum over chunks per
// output (vjp_reduce_steps_stage2).  dCfin, dcfin, dx0: one record per instance, vjp_reduce_final, then the chunks in
// order (vjp_reduce_steps_stage2 with T = 1).  dlow, dhigh: box_reduce_bounds per (chunk, step), box_reduce_final over
// chunks and steps.  No atomics: the same call gives the same bits.
//
// Workspace in elements of S, every array rounded up to 64: ct [B][T][d], cT [B][n], Cfe [B][n][n], zer [B][n],
// dS [B][T + 1][n], dA [B][T][m], dcost [B][T + 1] (VjpPrefix); the adjoint solve's own workspace; then
//   fp32:  P [B][T][2n], Pf [B][n], partial
//   fp64:  V [B][T][n][n], vt [B][T][n], P [B][T][2n], partial
// with partial [chunks][T][E], E = n d + n + d d + d (>= chunks n n of the final-cost sums); the control-limited VJP
// appends mask [B][T], Rlo and Rhi [B][T][m] (fp32; the double one states its longer tail at tvlqr_vjp_f64.hip's BoxLayout).
//
// The build is -ffp-contract=off: every fused multiply-add is a written fma().
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "tvlqr_kernels.h"

namespace tfmpc {

constexpr int kChunk = 256;          // instances per stage-1 partial sum
constexpr int kTile = 16;            // records per LDS tile in stage 1
constexpr int kRedThreads = 256;
constexpr int kEpt = 4;              // output elements per thread per pass in stage 1
constexpr int kWaveThreads = 64;     // one wavefront per (b, t), per instance or per (chunk, t)

enum Kind { kF = 0, kf, kC, kc, kCfin, kcfin, kx0, kKinds };

template <class S>
struct OutT {
    S *p;
    long sb, st;
};

// What the fold and the reductions read, and F, which only the fp32 sweep reads.  The double file's VjpArgs adds the
// operands of its costate kernel.  The order up to o[] is the fp32 argument block's from before the reductions were
// shared, a0 in the place of its dlam_0 records, and stays: the fp32 sweep kernels live at the SGPR limit, and moving
// their argument offsets changes their spill code (F at the tail: +0.7 % device time on box_sweep_kernel).
template <class S>
struct VjpBase {
    int B, n, m, T;
    const S *F, *C, *c;
    long sF_b, sF_t, sC_b, sC_t, sc_b, sc_t;
    const S *Cf, *cf;                // final cost (explicit, or the default's copy of C_{T-1}[:n,:n] and c_{T-1}[:n]); row stride n
    long sCf_b, scf_b;
    bool dflt;                       // default final cost: its gradients go into dC_{T-1}[:n,:n], dc_{T-1}[:n]
    const S *states, *actions, *gx, *gu, *gc;
    const S *dS, *dA, *ct, *cT;      // adjoint trajectory, c~, c~_fin
    const int32_t *status;
    S *P;                            // per (b, t): (dlam_{t+1}, lam_{t+1}) [2n]
    S *a0;                           // per b: dlam_0 [n], batch stride sa0_b (fp32: the sweep's records; double: v~_0)
    OutT<S> o[kKinds];
    long sa0_b;
    int32_t poison_mask;             // the status bits of the adjoint solve that make an instance NaN
};

// The control-limited VJP's extra operands.  fp32: Rlo doubles as the fold's record of the unmasked g_u (read by the
// sweep before it overwrites the entry with the bound's gradient); the double VJP (tvlqr_vjp_f64.hip's BoxArgs) hands
// the fold a record of its own in Rlo's place.
template <class S>
struct BoxArgsT {
    const S *low, *high;
    long slo_b, slo_t, shi_b, shi_t;
    uint32_t *mask, *mask_out;       // [B][T]: workspace, caller's (optional)
    S *Rlo, *Rhi;                    // [B][T][m]
    OutT<S> olo, ohi;
};

// The arguments of a C entry (include/tfmpc_hip.h), in the order the entries take them: what all four VJP entries
// share, and what the two control-limited ones add.
template <class S>
struct VjpCall {
    int B, n, m, T;
    const S *F; long sF_b, sF_t;
    const S *f; long sf_b, sf_t;
    const S *C; long sC_b, sC_t;
    const S *c; long sc_b, sc_t;
    const S *Cfin; long sCfin_b;
    const S *cfin; long scfin_b;
    const S *states, *actions, *g_states, *g_actions, *g_costs;
    S *dF; long sdF_b, sdF_t;
    S *df; long sdf_b, sdf_t;
    S *dC; long sdC_b, sdC_t;
    S *dc; long sdc_b, sdc_t;
    S *dCfin; long sdCfin_b;
    S *dcfin; long sdcfin_b;
    S *dx0; long sdx0_b;
    int32_t *status;
    void *workspace;
    size_t workspace_bytes;
    void *stream;
};

template <class S>
struct BoxCall {
    const S *low; long slo_b, slo_t;
    const S *high; long shi_b, shi_t;
    S *dlow; long sdlo_b, sdlo_t;
    S *dhigh; long sdhi_b, sdhi_t;
    uint32_t *clamp_mask;
};

__device__ inline bool same_bits(float x, float y) { return __float_as_uint(x) == __float_as_uint(y); }
__device__ inline bool same_bits(double x, double y) { return __double_as_longlong(x) == __double_as_longlong(y); }

template <class S>
__device__ inline S poison_of(const int32_t *status, int32_t mask, int b)
{
    return (status[b] & mask) ? S(__builtin_nanf("")) : S(0);
}

// ---- 1. fold -------------------------------------------------------------------------------------------------------
// One wavefront per (b, t); t == T is the final step (rows < n).  With a cost gradient, C_t is staged in LDS by
// coalesced loads (row stride d + 1) and each lane takes rows of C_t z_t + c_t.  BOX: also the held-set word per (b, t)
// -- a control whose bits equal low's or high's -- with the held entries of c~ zeroed and the unmasked g_u kept in Rlo.
template <class S, bool BOX>
__device__ __forceinline__ void fold_body(const VjpBase<S> &a, S *ct, S *cT, S *Cfe, S *zer, const BoxArgsT<S> *bx)
{
    extern __shared__ __attribute__((aligned(sizeof(double)))) unsigned char lds[];
    S *sm = reinterpret_cast<S *>(lds);
    const int n = a.n, m = a.m, T = a.T, d = n + m, L = threadIdx.x;
    const int b = (int)(blockIdx.x / (T + 1)), t = (int)(blockIdx.x % (T + 1));
    const S *x = a.states + ((size_t)b * (T + 1) + t) * n;
    if (t < T) {
        uint32_t held = 0;
        if constexpr (BOX) {         // lane i < m (m <= 32): is control i on a bound, bit for bit?
            bool on = false;
            if (L < m) {
                const S u = a.actions[((size_t)b * T + t) * m + L];
                on = same_bits(u, tv_at(bx->low, bx->slo_b, bx->slo_t, b, t)[L]) ||
                     same_bits(u, tv_at(bx->high, bx->shi_b, bx->shi_t, b, t)[L]);
            }
            held = (uint32_t)__ballot(on);
            if (L == 0) {
                bx->mask[(size_t)b * T + t] = held;
                if (bx->mask_out) bx->mask_out[(size_t)b * T + t] = held;
            }
        }
        S *sC = sm, *sz = sm + (size_t)d * (d + 1);
        if (a.gc) {
            const S *Ct = tv_at(a.C, a.sC_b, a.sC_t, b, t);
            for (int e = L; e < d * d; e += kWaveThreads) sC[(e / d) * (d + 1) + e % d] = Ct[e];
            const S *u = a.actions + ((size_t)b * T + t) * m;
            for (int i = L; i < d; i += kWaveThreads) sz[i] = i < n ? x[i] : u[i - n];
            __syncthreads();
        }
        for (int i = L; i < d; i += kWaveThreads) {
            S g = 0;
            if (i < n) { if (a.gx) g = a.gx[((size_t)b * (T + 1) + t) * n + i]; }
            else if (a.gu) g = a.gu[((size_t)b * T + t) * m + (i - n)];
            if (a.gc) {
                const S w = a.gc[(size_t)b * (T + 1) + t];
                const S *Ci = sC + (size_t)i * (d + 1);
                S r = tv_at(a.c, a.sc_b, a.sc_t, b, t)[i];
                for (int j = 0; j < d; ++j) r = fma(Ci[j], sz[j], r);
                g = fma(w, r, g);
            }
            if constexpr (BOX)
                if (i >= n) {
                    bx->Rlo[((size_t)b * T + t) * m + (i - n)] = g;
                    if (held >> (i - n) & 1u) g = 0;
                }
            ct[((size_t)b * T + t) * d + i] = g;
        }
        return;
    }
    for (int i = L; i < n; i += kWaveThreads) {
        zer[(size_t)b * n + i] = 0;
        const S *Crow;
        if (a.dflt) {                // C_{T-1}[i, :n]: copy the row into the adjoint's explicit final cost
            Crow = tv_at(a.C, a.sC_b, a.sC_t, b, T - 1) + (size_t)i * d;
            if (a.sCf_b != 0 || b == 0)
                for (int j = 0; j < n; ++j) Cfe[(size_t)b * a.sCf_b + (size_t)i * n + j] = Crow[j];
        } else {
            Crow = a.Cf + (size_t)b * a.sCf_b + (size_t)i * n;
        }
        S g = a.gx ? a.gx[((size_t)b * (T + 1) + T) * n + i] : S(0);
        if (a.gc) {
            S r = a.cf[(size_t)b * a.scf_b + i];
            for (int j = 0; j < n; ++j) r = fma(Crow[j], x[j], r);
            g = fma(a.gc[(size_t)b * (T + 1) + T], r, g);
        }
        cT[(size_t)b * n + i] = g;
    }
}

// ---- 4. batch reductions ---------------------------------------------------------------------------------------------
// A record of instance b: a[n] l[n] z[d] dz[d] gc.  Step records (t < T) take a = dlam_{t+1}, l = lam_{t+1}; the final
// record takes z[:n] = x_T, dz[:n] = dx_T, gc = gcost_T and a = dlam_0 (a.a0).
template <class S>
__device__ inline void load_record(const VjpBase<S> &a, S *rec, int b, int t, bool fin, int lane, int nthr)
{
    const int n = a.n, m = a.m, T = a.T, d = n + m, W = 2 * n + 2 * d + 1;
    const S poison = poison_of<S>(a.status, a.poison_mask, b);
    for (int q = lane; q < W; q += nthr) {
        S v;
        if (q < 2 * n) {
            if (fin) v = q < n ? a.a0[(size_t)b * a.sa0_b + q] : S(0);
            else v = a.P ? a.P[((size_t)b * T + t) * 2 * n + q] : S(0);
        } else if (q < 2 * n + d) {
            const int i = q - 2 * n;
            if (fin) v = i < n ? a.states[((size_t)b * (T + 1) + T) * n + i] : S(0);
            else v = i < n ? a.states[((size_t)b * (T + 1) + t) * n + i] : a.actions[((size_t)b * T + t) * m + i - n];
        } else if (q < 2 * n + 2 * d) {
            const int i = q - 2 * n - d;
            if (fin) v = i < n ? a.dS[((size_t)b * (T + 1) + T) * n + i] : S(0);
            else v = i < n ? a.dS[((size_t)b * (T + 1) + t) * n + i] : a.dA[((size_t)b * T + t) * m + i - n];
        } else {
            v = a.gc ? a.gc[(size_t)b * (T + 1) + (fin ? T : t)] : S(0);
        }
        rec[q] = v + poison;
    }
}

template <class S>
__device__ inline S contrib(int kind, const S *r, int n, int d, int e, bool fin_into_step)
{
    const S *al = r, *l = r + n, *z = r + 2 * n, *dz = z + d, gc = z[2 * d];
    switch (kind) {
    case kF: { const int i = e / d, j = e % d; return fma(al[i], z[j], l[i] * dz[j]); }
    case kf: return al[e];
    case kC: {
        const int i = e / d, j = e % d;
        if (fin_into_step && (i >= n || j >= n)) return S(0);
        return S(0.5) * (dz[i] * z[j] + z[i] * dz[j] + gc * z[i] * z[j]);
    }
    case kc: if (fin_into_step && e >= n) return S(0); return dz[e] + gc * z[e];
    case kCfin: { const int i = e / n, j = e % n; return S(0.5) * (dz[i] * z[j] + z[i] * dz[j] + gc * z[i] * z[j]); }
    case kcfin: return dz[e] + gc * z[e];
    default: return al[e];       // kx0
    }
}

// dCfin, dcfin, dx0 shared by the batch: the final records of a chunk of instances.  grid (chunks); partial[chunk * nE + e]
template <class S>
__global__ void __launch_bounds__(kRedThreads) vjp_reduce_final(VjpBase<S> a, int kind, int nE, S *partial)
{
    extern __shared__ __attribute__((aligned(sizeof(double)))) unsigned char lds[];
    S *tile = reinterpret_cast<S *>(lds);
    const int n = a.n, d = n + a.m, W = 2 * n + 2 * d + 1;
    const int chunk = blockIdx.x, tid = threadIdx.x;
    const int b0 = chunk * kChunk, b1 = min(a.B, b0 + kChunk);
    for (int e0 = 0; e0 < nE; e0 += kRedThreads * kEpt) {
        S acc[kEpt];
        for (int q = 0; q < kEpt; ++q) acc[q] = 0;
        for (int bb = b0; bb < b1; bb += kTile) {
            const int nb = min(kTile, b1 - bb);
            __syncthreads();
            for (int r = tid / 16; r < nb; r += kRedThreads / 16) load_record(a, tile + r * W, bb + r, 0, true, tid % 16, 16);
            __syncthreads();
            for (int r = 0; r < nb; ++r)
                for (int q = 0; q < kEpt; ++q) {
                    const int e = e0 + q * kRedThreads + tid;
                    if (e < nE) acc[q] += contrib(kind, tile + r * W, n, d, e, false);
                }
        }
        for (int q = 0; q < kEpt; ++q) {
            const int e = e0 + q * kRedThreads + tid;
            if (e < nE) partial[(size_t)chunk * nE + e] = acc[q];
        }
    }
}

// Bound gradients shared by the batch (the control-limited VJPs): partial[(chunk * T + t) * m + e] = sum over the chunk's
// instances of R[b][t][e], eight interleaved sub-sums per element combined in a fixed order (m <= 32).
template <class S>
__global__ void __launch_bounds__(kRedThreads) box_reduce_bounds(const S *R, int B, int T, int m, S *partial)
{
    __shared__ S sub[kRedThreads];
    const int chunk = blockIdx.x, t = blockIdx.y, e = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int b0 = chunk * kChunk, b1 = min(B, b0 + kChunk);
    S s = 0;
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
template <class S>
__global__ void __launch_bounds__(kRedThreads) box_reduce_final(const S *partial, int chunks, int T, int m, bool timed, S *out, long st)
{
    __shared__ S sub[kRedThreads];
    const int e = blockIdx.x, slot = blockIdx.y, tid = threadIdx.x;
    const int t0 = timed ? slot : 0, nt = timed ? 1 : T, total = chunks * nt;
    S s = 0;
    for (int q = tid; q < total; q += kRedThreads) s += partial[((size_t)(q / nt) * T + t0 + q % nt) * m + e];
    sub[tid] = s;
    __syncthreads();
    for (int w = kRedThreads / 2; w > 0; w >>= 1) {
        if (tid < w) sub[tid] += sub[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[(size_t)slot * st + e] = sub[0];
}

// Fused per-step reductions: ONE pass over the records emits every requested batch-shared per-step gradient (dF, df,
// dC, dc) of a chunk of instances at step t.  partial[(chunk * T + t) * E + off_k + e], E = n d + n + d d + d.
__host__ __device__ inline int steps_E(int n, int d) { return n * d + n + d * d + d; }
__host__ __device__ inline int steps_off(int k, int n, int d)
{
    return k == kF ? 0 : k == kf ? n * d : k == kC ? n * d + n : n * d + n + d * d;
}

// Shape-generic form: records staged in LDS tiles, scalar sums over the concatenated outputs.
template <class S>
__global__ void __launch_bounds__(kRedThreads) vjp_reduce_steps(VjpBase<S> a, unsigned need, S *partial)
{
    extern __shared__ __attribute__((aligned(sizeof(double)))) unsigned char lds[];
    S *tile = reinterpret_cast<S *>(lds);
    const int n = a.n, d = n + a.m, T = a.T, W = 2 * n + 2 * d + 1, E = steps_E(n, d);
    const int chunk = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int b0 = chunk * kChunk, b1 = min(a.B, b0 + kChunk);
    const int passes = (a.dflt && t == T - 1) ? 2 : 1;      // pass 1: the default final cost's records into dC, dc
    for (int e0 = 0; e0 < E; e0 += kRedThreads * kEpt) {
        S acc[kEpt];
        int kind[kEpt], ee[kEpt];
        for (int q = 0; q < kEpt; ++q) {
            acc[q] = 0;
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

// The 16x16x4 matrix-core instruction of S.  A / B operands: one S per lane in both precisions.  C/D: register r of
// lane (li = lane & 15, lq = lane >> 4) is column li of row(lq, r) -- the two maps differ (wave_ops_f64.h).
template <class S>
struct Mfma16;
template <>
struct Mfma16<float> {
    using Acc = __attribute__((ext_vector_type(4))) float;
    static __device__ __forceinline__ Acc mac(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lq, int r) { return 4 * lq + r; }
};
template <>
struct Mfma16<double> {
    using Acc = __attribute__((ext_vector_type(4))) double;
    static __device__ __forceinline__ Acc mac(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int lq, int r) { return lq + 4 * r; }
};

// n <= 16, d <= 32: the batch sums are GEMMs over instances on v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 (operands
// and accumulation in S), four instances per k-step, one wave per (chunk, t).  Lane (li = lane & 15, lq = lane >> 4)
// loads instance b0 + lq's entries li and 16 + li straight into the A / B operand slots:
//   dF = [dlam | lam] [z | dz]^T            (two 16 x 16 column tiles)
//   dC = ([dz | z] [z | dz + gc z]^T) / 2   (2 x 2 tiles)
// df and dc are per-lane sums, combined over the four k-groups in a fixed order.
template <class S>
__global__ void __launch_bounds__(kWaveThreads) vjp_reduce_steps_mfma16(VjpBase<S> a, unsigned need, S *partial)
{
    using M = Mfma16<S>;
    const int n = a.n, m = a.m, T = a.T, d = n + m, E = steps_E(n, d);
    const int chunk = blockIdx.x, t = blockIdx.y, lane = threadIdx.x, li = lane & 15, lq = lane >> 4;
    const int b0 = chunk * kChunk, b1 = min(a.B, b0 + kChunk);
    const bool wantF = need & ((1u << kF) | (1u << kf)), wantC = need & ((1u << kC) | (1u << kc));
    typename M::Acc F0 = {0, 0, 0, 0}, F1 = F0, C00 = F0, C01 = F0, C10 = F0, C11 = F0;
    S sf = 0, sc0 = 0, sc1 = 0;
    const int passes = (a.dflt && t == T - 1) ? 2 : 1;
    for (int pass = 0; pass < passes; ++pass) {
        const bool fin = pass == 1;
        const int ts = fin ? T : t;
        for (int bb = b0; bb < b1; bb += 4) {
            const int b = bb + lq;
            S av = 0, lv = 0, z0 = 0, z1 = 0, dz0 = 0, dz1 = 0, gc = 0;
            if (b < b1) {
                const S p = poison_of<S>(a.status, a.poison_mask, b);
                const S *x = a.states + ((size_t)b * (T + 1) + ts) * n, *dx = a.dS + ((size_t)b * (T + 1) + ts) * n;
                const S *u = a.actions + ((size_t)b * T + t) * m, *du = a.dA + ((size_t)b * T + t) * m;
                const int j1 = 16 + li;
                if (fin) {
                    if (li < n) { z0 = x[li]; dz0 = dx[li]; }
                } else {
                    if (wantF && li < n) {
                        const S *P = a.P + ((size_t)b * T + t) * 2 * n;
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
            const S w0 = fma(gc, z0, dz0), w1 = fma(gc, z1, dz1);
            if (wantF && !fin) {
                F0 = M::mac(av, z0, F0);
                F0 = M::mac(lv, dz0, F0);
                F1 = M::mac(av, z1, F1);
                F1 = M::mac(lv, dz1, F1);
                sf += av;
            }
            if (wantC) {
                C00 = M::mac(dz0, z0, C00);
                C00 = M::mac(z0, w0, C00);
                C01 = M::mac(dz0, z1, C01);
                C01 = M::mac(z0, w1, C01);
                C10 = M::mac(dz1, z0, C10);
                C10 = M::mac(z1, w0, C10);
                C11 = M::mac(dz1, z1, C11);
                C11 = M::mac(z1, w1, C11);
                sc0 += w0;
                sc1 += w1;
            }
        }
    }
    S *out = partial + ((size_t)chunk * T + t) * E;
    // the four k-groups of lane li, summed in a fixed order
    auto fold4 = [&](S v) {
        return ((__shfl(v, li) + __shfl(v, li + 16)) + __shfl(v, li + 32)) + __shfl(v, li + 48);
    };
    const S tf = fold4(sf), tc0 = fold4(sc0), tc1 = fold4(sc1);
    for (int r = 0; r < 4; ++r) {
        const int i = M::row(lq, r);
        if (i < n) {
            if (li < d) out[i * d + li] = F0[r];
            if (16 + li < d) out[i * d + 16 + li] = F1[r];
        }
        const int cb = steps_off(kC, n, d);
        if (i < d && li < d) out[cb + i * d + li] = S(0.5) * C00[r];
        if (i < d && 16 + li < d) out[cb + i * d + 16 + li] = S(0.5) * C01[r];
        if (16 + i < d && li < d) out[cb + (16 + i) * d + li] = S(0.5) * C10[r];
        if (16 + i < d && 16 + li < d) out[cb + (16 + i) * d + 16 + li] = S(0.5) * C11[r];
    }
    if (lq == 0) {
        if (li < n) out[steps_off(kf, n, d) + li] = tf;
        if (li < d) out[steps_off(kc, n, d) + li] = tc0;
        if (16 + li < d) out[steps_off(kc, n, d) + 16 + li] = tc1;
    }
}

// Stage 2: out[slot * st + e] = sum over chunks, then over the slot's steps, in that order.  The one-record-per-instance
// sums use it with T = 1, E = nE, off = 0: the chunks in order.
template <class S>
__global__ void vjp_reduce_steps_stage2(const S *partial, int chunks, int T, int E, int off, int nE, bool timed, S *out, long st)
{
    const int slots = timed ? T : 1;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)slots * nE) return;
    const int slot = (int)(idx / nE), e = (int)(idx % nE);
    const int t0 = timed ? slot : 0, t1 = timed ? slot + 1 : T;
    S s = 0;
    for (int k = 0; k < chunks; ++k)
        for (int t = t0; t < t1; ++t) s += partial[((size_t)k * T + t) * E + off + e];
    out[(size_t)slot * st + e] = s;
}

// Enqueues the sums of every gradient with batch stride 0: the per-step kinds in one pass and one short sum per output,
// then the final-record kinds one by one.  partial: [chunks][T][E] elements.
template <class S>
int vjp_shared_sums(const VjpBase<S> &a, S *partial, hipStream_t s)
{
    const int n = a.n, d = n + a.m, T = a.T, chunks = (a.B + kChunk - 1) / kChunk, W = 2 * n + 2 * d + 1;
    const int nEs[kKinds] = {n * d, n, d * d, d, n * n, n, n};
    unsigned need = 0;
    for (int k = kF; k <= kc; ++k)
        if (a.o[k].p && !a.o[k].sb) need |= 1u << k;
    if (need) {                      // dF, df, dC, dc: one pass over the records, then one short sum per output
        if (n <= 16 && d <= 32)
            hipLaunchKernelGGL(vjp_reduce_steps_mfma16<S>, dim3(chunks, T), dim3(kWaveThreads), 0, s, a, need, partial);
        else
            hipLaunchKernelGGL(vjp_reduce_steps<S>, dim3(chunks, T), dim3(kRedThreads), (size_t)kTile * W * sizeof(S), s, a, need,
                               partial);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
        for (int k = kF; k <= kc; ++k) {
            if (!(need >> k & 1u)) continue;
            const bool timed = a.o[k].st != 0;
            const size_t total = (size_t)(timed ? T : 1) * nEs[k];
            hipLaunchKernelGGL(vjp_reduce_steps_stage2<S>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, partial, chunks,
                               T, steps_E(n, d), steps_off(k, n, d), nEs[k], timed, a.o[k].p, a.o[k].st);
            if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
        }
    }
    for (int k = kCfin; k < kKinds; ++k) {      // final-cost and x0 sums: one record per instance, the chunks in order
        const OutT<S> &o = a.o[k];
        if (!o.p || o.sb) continue;
        hipLaunchKernelGGL(vjp_reduce_final<S>, dim3(chunks), dim3(kRedThreads), (size_t)kTile * W * sizeof(S), s, a, k, nEs[k],
                           partial);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
        hipLaunchKernelGGL(vjp_reduce_steps_stage2<S>, dim3((unsigned)((nEs[k] + 255) / 256)), dim3(256), 0, s, partial, chunks, 1,
                           nEs[k], 0, nEs[k], false, o.p, 0L);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    return TFMPC_OK;
}

// Enqueues the sums of dlow / dhigh where the batch shares them: the records per (b, t), chunks, then steps.
template <class S>
int box_shared_sums(const BoxArgsT<S> &bx, int B, int T, int m, S *partial, hipStream_t s)
{
    const int chunks = (B + kChunk - 1) / kChunk;
    const OutT<S> bo[2] = {bx.olo, bx.ohi};
    const S *rec[2] = {bx.Rlo, bx.Rhi};
    for (int k = 0; k < 2; ++k) {
        if (!bo[k].p || bo[k].sb) continue;
        hipLaunchKernelGGL(box_reduce_bounds<S>, dim3(chunks, T), dim3(kRedThreads), 0, s, rec[k], B, T, m, partial);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
        const bool timed = bo[k].st != 0;
        hipLaunchKernelGGL(box_reduce_final<S>, dim3(m, timed ? T : 1), dim3(kRedThreads), 0, s, partial, chunks, T, m, timed,
                           bo[k].p, bo[k].st);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    return TFMPC_OK;
}

// ---- workspace -------------------------------------------------------------------------------------------------------
inline size_t fold_smem_elems(int n, int m) { const size_t d = n + m; return d * (d + 1) + d; }

inline size_t up64(size_t x) { return (x + 63) / 64 * 64; }

struct VjpPrefix { size_t ct, cT, Cfe, zer, dS, dA, dcost; };     // offsets in elements

// Fills the offsets of the arrays both precisions start with; returns the offset after them.
inline size_t vjp_prefix(VjpPrefix &L, int B, int n, int m, int T)
{
    const size_t d = n + m, Bs = B, Ts = T;
    size_t o = 0;
    L.ct = o; o += up64(Bs * Ts * d);
    L.cT = o; o += up64(Bs * n);
    L.Cfe = o; o += up64(Bs * n * n);
    L.zer = o; o += up64(Bs * n);
    L.dS = o; o += up64(Bs * (Ts + 1) * n);
    L.dA = o; o += up64(Bs * Ts * m);
    L.dcost = o; o += up64(Bs * (Ts + 1));
    return o;
}

// the partial sums of the reductions: >= chunks * n * n of the final-cost sums
inline size_t vjp_partial_elems(int B, int n, int m, int T)
{
    return up64(((size_t)B + kChunk - 1) / kChunk * T * (size_t)steps_E(n, n + m));
}

// The plain double VJP around its adjoint solve (tvlqr_vjp_f64.hip), for a caller that brings the adjoint trajectory itself
// (tvlqr_vjp_time_parallel_f64.hip); w: the caller's workspace, which starts with VjpPrefix.  The fold fills
// ct, cT, Cfe, zer.  The costates and batch sums read dS, dA, the forward's v [B][T][n], V [B][T][n][n] and v~ [B][T][n] of the
// adjoint problem, and use P [B][T][2n] and partial (vjp_partial_elems) as scratch.
int tvlqr_vjp_f64_fold_launch(const VjpCall<double> &c, double *w, const VjpPrefix &L);
int tvlqr_vjp_f64_costates_launch(const VjpCall<double> &c, double *w, const VjpPrefix &L, const double *v, const double *V,
                                  const double *vt, double *P, double *partial);

// ---- the argument contract of the four entries -------------------------------------------------------------------------
// The checks that follow an entry's own shape test and its B == 0 return, in the order every entry has always made them.
// fits: the precision's own refusals (LDS sizes, the held-set word), which come after the grid limits and before the
// bounds' operands.
template <class S>
int vjp_check_call(const VjpCall<S> &c, const BoxCall<S> *box, bool fits)
{
    if (!c.F || !c.f || !c.C || !c.c || !c.states || !c.actions || !c.status) return TFMPC_ERR_ARG;
    if (!c.Cfin != !c.cfin) return TFMPC_ERR_ARG;
    if (!c.Cfin && (c.dCfin || c.dcfin)) return TFMPC_ERR_ARG;     // the default final cost's gradient is in dC, dc
    if (c.T > 65535) return TFMPC_ERR_UNSUPPORTED;                 // per-step reduction slots are one grid axis
    if ((size_t)c.B * (c.T + 1) > 0x7fffffffu) return TFMPC_ERR_UNSUPPORTED;   // fold (double: costates too): one block per (b, t)
    if (!fits) return TFMPC_ERR_UNSUPPORTED;
    if (box) {
        if (!box->low || !box->high) return TFMPC_ERR_ARG;
        for (long s : {box->slo_b, box->slo_t, box->shi_b, box->shi_t, box->sdlo_b, box->sdlo_t, box->sdhi_b, box->sdhi_t})
            if (s < 0) return TFMPC_ERR_ARG;
    }
    for (long s : {c.sF_b, c.sF_t, c.sf_b, c.sf_t, c.sC_b, c.sC_t, c.sc_b, c.sc_t, c.sCfin_b, c.scfin_b, c.sdF_b, c.sdF_t, c.sdf_b,
                   c.sdf_t, c.sdC_b, c.sdC_t, c.sdc_b, c.sdc_t, c.sdCfin_b, c.sdcfin_b, c.sdx0_b})
        if (s < 0) return TFMPC_ERR_ARG;
    return TFMPC_OK;
}

// What of VjpBase<S> does not depend on the precision's costates: the model, the final cost, the trajectory, the upstream
// gradients, the adjoint's arrays in the workspace w, the outputs and the status.  P, a0 and poison_mask are the caller's.
template <class S>
void vjp_fill_base(VjpBase<S> &a, const VjpCall<S> &c, S *w, const VjpPrefix &L)
{
    a.B = c.B; a.n = c.n; a.m = c.m; a.T = c.T;
    a.F = c.F; a.sF_b = c.sF_b; a.sF_t = c.sF_t;
    a.C = c.C; a.sC_b = c.sC_b; a.sC_t = c.sC_t;
    a.c = c.c; a.sc_b = c.sc_b; a.sc_t = c.sc_t;
    a.dflt = c.Cfin == nullptr;
    a.states = c.states; a.actions = c.actions; a.gx = c.g_states; a.gu = c.g_actions; a.gc = c.g_costs;
    a.dS = w + L.dS; a.dA = w + L.dA; a.ct = w + L.ct; a.cT = w + L.cT;
    a.status = c.status;
    if (a.dflt) {                    // the fold's copy of C_{T-1}[:n,:n]; c_{T-1}[:n], contiguous in c
        a.Cf = w + L.Cfe; a.sCf_b = c.sC_b ? (long)c.n * c.n : 0;
        a.cf = c.c + (size_t)(c.T - 1) * c.sc_t; a.scf_b = c.sc_b;
    } else {
        a.Cf = c.Cfin; a.sCf_b = c.sCfin_b;
        a.cf = c.cfin; a.scf_b = c.scfin_b;
    }
    const OutT<S> outs[kKinds] = {{c.dF, c.sdF_b, c.sdF_t}, {c.df, c.sdf_b, c.sdf_t}, {c.dC, c.sdC_b, c.sdC_t}, {c.dc, c.sdc_b, c.sdc_t},
                                  {c.dCfin, c.sdCfin_b, 0}, {c.dcfin, c.sdcfin_b, 0}, {c.dx0, c.sdx0_b, 0}};
    for (int k = 0; k < kKinds; ++k) a.o[k] = outs[k];
}

// The bounds' operands; mask, Rlo, Rhi: the caller's places in its workspace.
template <class S>
void box_fill(BoxArgsT<S> &bx, const BoxCall<S> &box, uint32_t *mask, S *Rlo, S *Rhi)
{
    bx.low = box.low; bx.slo_b = box.slo_b; bx.slo_t = box.slo_t;
    bx.high = box.high; bx.shi_b = box.shi_b; bx.shi_t = box.shi_t;
    bx.mask = mask; bx.mask_out = box.clamp_mask;
    bx.Rlo = Rlo; bx.Rhi = Rhi;
    bx.olo = OutT<S>{box.dlow, box.sdlo_b, box.sdlo_t};
    bx.ohi = OutT<S>{box.dhigh, box.sdhi_b, box.sdhi_t};
}

}  // namespace tfmpc
