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
//   4. vjp_reduce_*         gradients with batch stride 0, as tvlqr_vjp.hip: one pass per (chunk of instances, step) --
//                           GEMMs over instances on v_mfma_f64_16x16x4_f64 for n <= 16, d <= 32, LDS-tiled scalar sums
//                           otherwise -- then the chunks (and steps) in a fixed order.
// An instance whose adjoint solve sets a status bit contributes NaN (its own rows, and every batch sum that includes it).
// The build is -ffp-contract=off: every fused multiply-add is a written fma().  No scratch memory.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "tvlqr_kernels.h"

using namespace tfmpc;

namespace {

constexpr int kChunk = 256;          // instances per stage-1 partial sum
constexpr int kTile = 16;            // records per LDS tile in stage 1
constexpr int kRedThreads = 256;
constexpr int kEpt = 4;              // output elements per thread per pass in stage 1
constexpr int kWaveThreads = 64;     // one wavefront per (b, t) or per instance

enum Kind { kF = 0, kf, kC, kc, kCfin, kcfin, kx0, kKinds };

struct Out {
    double *p;
    long sb, st;
};

struct VjpArgs {
    int B, n, m, T;
    const double *C, *c;             // the fold's operands (the costate kernel reads neither)
    long sC_b, sC_t, sc_b, sc_t;
    const double *Cf, *cf;           // V_T, v_T: the final cost (explicit, or the default's copy and c_{T-1}[:n]); row stride n
    long sCf_b, scf_b;
    bool dflt;                       // default final cost: its gradients go into dC_{T-1}[:n,:n], dc_{T-1}[:n]
    const double *states, *actions, *v, *gx, *gu, *gc;
    const double *dS, *dA, *ct, *cT; // adjoint trajectory, c~, c~_fin = v~_T
    const double *V, *vt;            // the adjoint solve's V[B][T][n][n], v~[B][T][n]
    const int32_t *status;
    double *P;                       // per (b, t): (dlam_{t+1}, lam_{t+1}) [2n]
    Out o[kKinds];
};

__device__ inline double poison_of(const int32_t *status, int b)
{
    return status[b] ? __builtin_nan("") : 0.0;
}

// ---- 1. fold -------------------------------------------------------------------------------------------------------
// One wavefront per (b, t); t == T is the final step (rows < n).  With a cost gradient, C_t is staged in LDS by
// coalesced loads (row stride d + 1) and each lane takes rows of C_t z_t + c_t.
__global__ void __launch_bounds__(kWaveThreads) vjp_fold_kernel(VjpArgs a, double *ct, double *cT, double *Cfe, double *zer)
{
    extern __shared__ double sm[];
    const int n = a.n, m = a.m, T = a.T, d = n + m, L = threadIdx.x;
    const int b = (int)(blockIdx.x / (T + 1)), t = (int)(blockIdx.x % (T + 1));
    const double *x = a.states + ((size_t)b * (T + 1) + t) * n;
    if (t < T) {
        double *sC = sm, *sz = sm + (size_t)d * (d + 1);
        if (a.gc) {
            const double *Ct = tv_at(a.C, a.sC_b, a.sC_t, b, t);
            for (int e = L; e < d * d; e += kWaveThreads) sC[(e / d) * (d + 1) + e % d] = Ct[e];
            const double *u = a.actions + ((size_t)b * T + t) * m;
            for (int i = L; i < d; i += kWaveThreads) sz[i] = i < n ? x[i] : u[i - n];
            __syncthreads();
        }
        for (int i = L; i < d; i += kWaveThreads) {
            double g = 0.0;
            if (i < n) { if (a.gx) g = a.gx[((size_t)b * (T + 1) + t) * n + i]; }
            else if (a.gu) g = a.gu[((size_t)b * T + t) * m + (i - n)];
            if (a.gc) {
                const double w = a.gc[(size_t)b * (T + 1) + t];
                const double *Ci = sC + (size_t)i * (d + 1);
                double r = tv_at(a.c, a.sc_b, a.sc_t, b, t)[i];
                for (int j = 0; j < d; ++j) r = fma(Ci[j], sz[j], r);
                g = fma(w, r, g);
            }
            ct[((size_t)b * T + t) * d + i] = g;
        }
        return;
    }
    for (int i = L; i < n; i += kWaveThreads) {
        zer[(size_t)b * n + i] = 0.0;
        const double *Crow;
        if (a.dflt) {                // C_{T-1}[i, :n]: copy the row into the adjoint's explicit final cost
            Crow = tv_at(a.C, a.sC_b, a.sC_t, b, T - 1) + (size_t)i * d;
            if (a.sCf_b != 0 || b == 0)
                for (int j = 0; j < n; ++j) Cfe[(size_t)b * a.sCf_b + (size_t)i * n + j] = Crow[j];
        } else {
            Crow = a.Cf + (size_t)b * a.sCf_b + (size_t)i * n;
        }
        double g = a.gx ? a.gx[((size_t)b * (T + 1) + T) * n + i] : 0.0;
        if (a.gc) {
            double r = a.cf[(size_t)b * a.scf_b + i];
            for (int j = 0; j < n; ++j) r = fma(Crow[j], x[j], r);
            g = fma(a.gc[(size_t)b * (T + 1) + T], r, g);
        }
        cT[(size_t)b * n + i] = g;
    }
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

// want: bit k = emit output k here.  LOOP = false: grid B T, block (b, t), every emitted output has its own slot per
// step (or T == 1).  LOOP = true: grid B, the block walks the steps backwards and accumulates in the output.
template <bool LOOP>
__global__ void __launch_bounds__(kWaveThreads) vjp_costate_kernel(VjpArgs a, unsigned want, bool store_factors)
{
    extern __shared__ double sm[];
    const int n = a.n, m = a.m, T = a.T, d = n + m, L = threadIdx.x;
    const int b = LOOP ? (int)blockIdx.x : (int)(blockIdx.x / T);
    double *sV = sm, *x1 = sV + (size_t)n * (n + 1), *dx1 = x1 + n, *lam = dx1 + n, *dlam = lam + n, *z = dlam + n, *dz = z + d;
    const double poison = poison_of(a.status, b);
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

// ---- 4. batch reductions ---------------------------------------------------------------------------------------------
// A record of instance b: a[n] l[n] z[d] dz[d] gc.  Step records (t < T) take a = dlam_{t+1}, l = lam_{t+1}; the final
// record takes z[:n] = x_T, dz[:n] = dx_T, gc = gcost_T and a = dlam_0 = v~_0.
__device__ inline void load_record(const VjpArgs &a, double *rec, int b, int t, bool fin, int lane, int nthr)
{
    const int n = a.n, m = a.m, T = a.T, d = n + m, W = 2 * n + 2 * d + 1;
    const double poison = poison_of(a.status, b);
    for (int q = lane; q < W; q += nthr) {
        double v;
        if (q < 2 * n) {
            if (fin) v = q < n ? a.vt[(size_t)b * T * n + q] : 0.0;
            else v = a.P ? a.P[((size_t)b * T + t) * 2 * n + q] : 0.0;
        } else if (q < 2 * n + d) {
            const int i = q - 2 * n;
            if (fin) v = i < n ? a.states[((size_t)b * (T + 1) + T) * n + i] : 0.0;
            else v = i < n ? a.states[((size_t)b * (T + 1) + t) * n + i] : a.actions[((size_t)b * T + t) * m + i - n];
        } else if (q < 2 * n + 2 * d) {
            const int i = q - 2 * n - d;
            if (fin) v = i < n ? a.dS[((size_t)b * (T + 1) + T) * n + i] : 0.0;
            else v = i < n ? a.dS[((size_t)b * (T + 1) + t) * n + i] : a.dA[((size_t)b * T + t) * m + i - n];
        } else {
            v = a.gc ? a.gc[(size_t)b * (T + 1) + (fin ? T : t)] : 0.0;
        }
        rec[q] = v + poison;
    }
}

__device__ inline double contrib(int kind, const double *r, int n, int d, int e, bool fin_into_step)
{
    const double *al = r, *l = r + n, *z = r + 2 * n, *dz = z + d, gc = z[2 * d];
    switch (kind) {
    case kF: { const int i = e / d, j = e % d; return fma(al[i], z[j], l[i] * dz[j]); }
    case kf: return al[e];
    case kC: {
        const int i = e / d, j = e % d;
        if (fin_into_step && (i >= n || j >= n)) return 0.0;
        return 0.5 * (dz[i] * z[j] + z[i] * dz[j] + gc * z[i] * z[j]);
    }
    case kc: if (fin_into_step && e >= n) return 0.0; return dz[e] + gc * z[e];
    case kCfin: { const int i = e / n, j = e % n; return 0.5 * (dz[i] * z[j] + z[i] * dz[j] + gc * z[i] * z[j]); }
    case kcfin: return dz[e] + gc * z[e];
    default: return al[e];       // kx0
    }
}

// dCfin, dcfin, dx0 shared by the batch: the final records of a chunk of instances.  grid (chunks); partial[chunk * nE + e]
__global__ void __launch_bounds__(kRedThreads) vjp_reduce_final(VjpArgs a, int kind, int nE, double *partial)
{
    extern __shared__ double tile[];
    const int n = a.n, d = n + a.m, W = 2 * n + 2 * d + 1;
    const int chunk = blockIdx.x, tid = threadIdx.x;
    const int b0 = chunk * kChunk, b1 = min(a.B, b0 + kChunk);
    for (int e0 = 0; e0 < nE; e0 += kRedThreads * kEpt) {
        double acc[kEpt];
        for (int q = 0; q < kEpt; ++q) acc[q] = 0.0;
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

// Fused per-step reductions: ONE pass over the records emits every requested batch-shared per-step gradient (dF, df,
// dC, dc) of a chunk of instances at step t.  partial[(chunk * T + t) * E + off_k + e], E = n d + n + d d + d.
__host__ __device__ inline int steps_E(int n, int d) { return n * d + n + d * d + d; }
__host__ __device__ inline int steps_off(int k, int n, int d)
{
    return k == kF ? 0 : k == kf ? n * d : k == kC ? n * d + n : n * d + n + d * d;
}

// Shape-generic form: records staged in LDS tiles, scalar sums over the concatenated outputs.
__global__ void __launch_bounds__(kRedThreads) vjp_reduce_steps(VjpArgs a, unsigned need, double *partial)
{
    extern __shared__ double tile[];
    const int n = a.n, d = n + a.m, T = a.T, W = 2 * n + 2 * d + 1, E = steps_E(n, d);
    const int chunk = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int b0 = chunk * kChunk, b1 = min(a.B, b0 + kChunk);
    const int passes = (a.dflt && t == T - 1) ? 2 : 1;      // pass 1: the default final cost's records into dC, dc
    for (int e0 = 0; e0 < E; e0 += kRedThreads * kEpt) {
        double acc[kEpt];
        int kind[kEpt], ee[kEpt];
        for (int q = 0; q < kEpt; ++q) {
            acc[q] = 0.0;
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

// n <= 16, d <= 32: the batch sums are GEMMs over instances on v_mfma_f64_16x16x4_f64, four instances per k-step, one
// wave per (chunk, t).  Lane (li = lane & 15, lq = lane >> 4) loads instance b0 + lq's entries li and 16 + li straight
// into the A / B operand slots (the f32 16x16x4 instruction's):
//   dF = [dlam | lam] [z | dz]^T            (two 16 x 16 column tiles)
//   dC = ([dz | z] [z | dz + gc z]^T) / 2   (2 x 2 tiles)
// The C/D map is the f64 instruction's own: register r of lane l is row lq + 4 r, column li (wave_ops_f64.h).  df and dc
// are per-lane sums, combined over the four k-groups in a fixed order.
__global__ void __launch_bounds__(kWaveThreads) vjp_reduce_steps_mfma16(VjpArgs a, unsigned need, double *partial)
{
    using f64x4 = __attribute__((ext_vector_type(4))) double;
    const int n = a.n, m = a.m, T = a.T, d = n + m, E = steps_E(n, d);
    const int chunk = blockIdx.x, t = blockIdx.y, lane = threadIdx.x, li = lane & 15, lq = lane >> 4;
    const int b0 = chunk * kChunk, b1 = min(a.B, b0 + kChunk);
    const bool wantF = need & ((1u << kF) | (1u << kf)), wantC = need & ((1u << kC) | (1u << kc));
    f64x4 F0 = {0, 0, 0, 0}, F1 = F0, C00 = F0, C01 = F0, C10 = F0, C11 = F0;
    double sf = 0.0, sc0 = 0.0, sc1 = 0.0;
    const int passes = (a.dflt && t == T - 1) ? 2 : 1;
    for (int pass = 0; pass < passes; ++pass) {
        const bool fin = pass == 1;
        const int ts = fin ? T : t;
        for (int bb = b0; bb < b1; bb += 4) {
            const int b = bb + lq;
            double av = 0.0, lv = 0.0, z0 = 0.0, z1 = 0.0, dz0 = 0.0, dz1 = 0.0, gc = 0.0;
            if (b < b1) {
                const double p = poison_of(a.status, b);
                const double *x = a.states + ((size_t)b * (T + 1) + ts) * n, *dx = a.dS + ((size_t)b * (T + 1) + ts) * n;
                const double *u = a.actions + ((size_t)b * T + t) * m, *du = a.dA + ((size_t)b * T + t) * m;
                const int j1 = 16 + li;
                if (fin) {
                    if (li < n) { z0 = x[li]; dz0 = dx[li]; }
                } else {
                    if (wantF && li < n) {
                        const double *P = a.P + ((size_t)b * T + t) * 2 * n;
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
            const double w0 = fma(gc, z0, dz0), w1 = fma(gc, z1, dz1);
            if (wantF && !fin) {
                F0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, z0, F0, 0, 0, 0);
                F0 = __builtin_amdgcn_mfma_f64_16x16x4f64(lv, dz0, F0, 0, 0, 0);
                F1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, z1, F1, 0, 0, 0);
                F1 = __builtin_amdgcn_mfma_f64_16x16x4f64(lv, dz1, F1, 0, 0, 0);
                sf += av;
            }
            if (wantC) {
                C00 = __builtin_amdgcn_mfma_f64_16x16x4f64(dz0, z0, C00, 0, 0, 0);
                C00 = __builtin_amdgcn_mfma_f64_16x16x4f64(z0, w0, C00, 0, 0, 0);
                C01 = __builtin_amdgcn_mfma_f64_16x16x4f64(dz0, z1, C01, 0, 0, 0);
                C01 = __builtin_amdgcn_mfma_f64_16x16x4f64(z0, w1, C01, 0, 0, 0);
                C10 = __builtin_amdgcn_mfma_f64_16x16x4f64(dz1, z0, C10, 0, 0, 0);
                C10 = __builtin_amdgcn_mfma_f64_16x16x4f64(z1, w0, C10, 0, 0, 0);
                C11 = __builtin_amdgcn_mfma_f64_16x16x4f64(dz1, z1, C11, 0, 0, 0);
                C11 = __builtin_amdgcn_mfma_f64_16x16x4f64(z1, w1, C11, 0, 0, 0);
                sc0 += w0;
                sc1 += w1;
            }
        }
    }
    double *out = partial + ((size_t)chunk * T + t) * E;
    // the four k-groups of lane li, summed in a fixed order
    auto fold4 = [&](double v) {
        return ((__shfl(v, li) + __shfl(v, li + 16)) + __shfl(v, li + 32)) + __shfl(v, li + 48);
    };
    const double tf = fold4(sf), tc0 = fold4(sc0), tc1 = fold4(sc1);
    for (int r = 0; r < 4; ++r) {
        const int i = lq + 4 * r;
        if (i < n) {
            if (li < d) out[i * d + li] = F0[r];
            if (16 + li < d) out[i * d + 16 + li] = F1[r];
        }
        const int cb = steps_off(kC, n, d);
        if (i < d && li < d) out[cb + i * d + li] = 0.5 * C00[r];
        if (i < d && 16 + li < d) out[cb + i * d + 16 + li] = 0.5 * C01[r];
        if (16 + i < d && li < d) out[cb + (16 + i) * d + li] = 0.5 * C10[r];
        if (16 + i < d && 16 + li < d) out[cb + (16 + i) * d + 16 + li] = 0.5 * C11[r];
    }
    if (lq == 0) {
        if (li < n) out[steps_off(kf, n, d) + li] = tf;
        if (li < d) out[steps_off(kc, n, d) + li] = tc0;
        if (16 + li < d) out[steps_off(kc, n, d) + 16 + li] = tc1;
    }
}

// Stage 2: out[slot * st + e] = sum over chunks, then over the slot's steps, in that order.  The one-record-per-instance
// sums use it with T = 1, E = nE, off = 0: the chunks in order, as batch_sum.h's in-order stage 2 (which is fp32).
__global__ void vjp_reduce_steps_stage2(const double *partial, int chunks, int T, int E, int off, int nE, bool timed,
                                        double *out, long st)
{
    const int slots = timed ? T : 1;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)slots * nE) return;
    const int slot = (int)(idx / nE), e = (int)(idx % nE);
    const int t0 = timed ? slot : 0, t1 = timed ? slot + 1 : T;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k)
        for (int t = t0; t < t1; ++t) s += partial[((size_t)k * T + t) * E + off + e];
    out[(size_t)slot * st + e] = s;
}

// ---- launch helpers --------------------------------------------------------------------------------------------------
size_t fold_smem_bytes(int n, int m) { const size_t d = n + m; return (d * (d + 1) + d) * sizeof(double); }

// ---- workspace -------------------------------------------------------------------------------------------------------
struct Layout {
    size_t ct, cT, Cfe, zer, dS, dA, dcost, solve, V, vt, P, partial, total;   // offsets in doubles
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
    L.solve_bytes = tfmpc_tvlqr_workspace_bytes_f64(B, n, m, T);
    L.solve = o; o += up64(L.solve_bytes / sizeof(double));
    L.V = o; o += up64(Bs * Ts * n * n);
    L.vt = o; o += up64(Bs * Ts * n);
    L.P = o; o += up64(Bs * Ts * 2 * n);
    L.partial = o; o += up64(chunks * Ts * (size_t)steps_E(n, (int)d));   // >= chunks * n * n of the final-cost sums
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
    a.status = status;
    a.P = w + L.P;
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
    hipLaunchKernelGGL(vjp_fold_kernel, dim3((unsigned)((size_t)B * (T + 1))), dim3(kWaveThreads), fold_smem_bytes(n, m), s, a,
                       w + L.ct, w + L.cT, w + L.Cfe, w + L.zer);
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
    const int chunks = (B + kChunk - 1) / kChunk;
    const int W = 2 * n + 2 * d + 1;
    const int nEs[kKinds] = {n * d, n, d * d, d, n * n, n, n};
    double *partial = w + L.partial;
    unsigned need = 0;
    for (int k = kF; k <= kc; ++k)
        if (a.o[k].p && !a.o[k].sb) need |= 1u << k;
    if (need) {                      // dF, df, dC, dc: one pass over the records, then one short sum per output
        if (n <= 16 && d <= 32)
            hipLaunchKernelGGL(vjp_reduce_steps_mfma16, dim3(chunks, T), dim3(kWaveThreads), 0, s, a, need, partial);
        else
            hipLaunchKernelGGL(vjp_reduce_steps, dim3(chunks, T), dim3(kRedThreads), (size_t)kTile * W * sizeof(double), s, a,
                               need, partial);
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
    for (int k = kCfin; k < kKinds; ++k) {      // final-cost and x0 sums: one record per instance, the chunks in order
        const Out &o = a.o[k];
        if (!o.p || o.sb) continue;
        hipLaunchKernelGGL(vjp_reduce_final, dim3(chunks), dim3(kRedThreads), (size_t)kTile * W * sizeof(double), s, a, k,
                           nEs[k], partial);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
        hipLaunchKernelGGL(vjp_reduce_steps_stage2, dim3((unsigned)((nEs[k] + 255) / 256)), dim3(256), 0, s, partial, chunks,
                           1, nEs[k], 0, nEs[k], false, o.p, 0L);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    return TFMPC_OK;
}

}  // extern "C"
