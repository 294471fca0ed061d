// tvlqr_mfma16x8.hip -- TIME-VARYING LQR backward + forward for n <= 16, m <= 8 on gfx950 matrix cores
// (tfmpc_tvlqr_*_f32, include/tfmpc_hip.h).  Smaller shapes are zero-padded to 16 x 8 exactly as in
// lqr_mfma16x8.hip (EXACT = false): zero rows / columns of F~ and C~, a unit diagonal on the padded part
// of C_uu, padded gains exactly 0.
//
// The per-step arithmetic is that of lqr_mfma16x8.hip: W = V F~_t and the three tiles of
// Q~ = C~_t + F~_t^T W as bf16x3 on v_mfma_f32_16x16x32_bf16 (TFMPC_LQR_MFMA=f32: v_mfma_f32_16x16x4_f32),
// the wave_ldlt8.h elimination, the Schur-form V' = Q_xx + Q_xu K on the f32 MFMA, V' symmetrised.
// What differs is where F~ and C~ come from: they are NOT resident, they arrive every step.
//
// Streaming: the backward sweep keeps TWO register sets of raw fp32 operands, 20 values per
// lane (F~_t two B-fragments, C~_t three tiles).  At the top of step t the loads of step t-1 are issued into
// the second set; step t then computes from the first; the sets swap at the bottom, where the only wait for
// the loads sits -- one whole step of MFMA / elimination work after they were issued.  A register set and not
// an LDS ring filled by global_load_lds: the operands are consumed in matrix-core operand layout, one value per
// lane per tile row, which is exactly the layout a plain per-lane global load produces; staging through LDS
// would add a ds_read per value and an LDS slice per wave for no reuse.
// The rollout streams F_t, f_t (ring of four steps, together with the gains) and, in the chunk epilogue,
// C_t, c_t for the stage costs (one step ahead).
#include <hip/hip_runtime.h>

#include "tvlqr_kernels.h"
#include "options.h"
#include "mfma_bf16x3.h"
#include "wave_ldlt8.h"
#include "wave_ops.h"

namespace tfmpc {

namespace {

constexpr int N = 16, M = 8, D = 24;
using f32x4 = bf3::f32x4;
using namespace bf3;

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float readlane(float v, int lane)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

template <int CTRL>
__device__ __forceinline__ float dpp(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141;

// per-wave LDS slice (floats), as lqr_mfma16x8.hip
constexpr int kMs = 0;          // [32 cols][8 rows]  elimination input, column-major
constexpr int kKs = 256;        // [32 cols][8 rows]  K~ = -Q_uu^-1 [Q_ux | . | q_u]
constexpr int kZs = 512;        // rollout chunk rows z_t = [x_t(16); u_t(8)], stride kZld (sweep: V' transpose staging)
constexpr int kZld = 26;
constexpr int kVtLd = 20;
constexpr int kTC = 52;         // timesteps per rollout chunk
constexpr int kLdsFloats = kZs + (kTC + 1) * kZld + 6;
constexpr int kRing = 4;        // rollout: steps of gains and dynamics in flight
static_assert(kTC % kRing == 0, "a chunk must hold whole turns of the ring");

// One step's operands of the sweep in matrix-core operand layout (lane (i, q), r = 0..3, k = 4q + r):
//   F0[r] = F~[k][i] (x columns), F1[r] = F~[k][16 + i] (u columns, f in column 24),
//   C00[r] = C~[k][i], C01t[r] = C_ux[k][i] (k < 8) | c_x[i] (k == 8), C11[r] = [C_uu | c_u][k][i].
struct StepOps { float F0[4], F1[4]; f32x4 C00, C01t, C11; };

// EXACT: n == 16, m == 8.  BF3: bf16x3 products.  VALUE: V, v, const outputs.
// Register budget: four waves per SIMD (<= 128 VGPRs) for the exact shape; the padded instantiations carry the guards and
// index maps of every streamed load, and the fused solve with value outputs carries both phases' state: at 128 they
// would spill, so they are sized for three (tests/test_tvlqr_cpu.py pins "no scratch" on every instantiation).
#define TFMPC_TVLQR_EU ((EXACT && !(VALUE && FORWARD)) ? 4 : 3)
// MASKED: the sweep of a model whose held controls (bit i of a.mask[b][t]) are taken out -- column
// 16 + i of F~_t zero, row and column 16 + i of C~_t zero with a unit diagonal, c_u[i] zero, the device that pads small
// shapes -- applied to the operand registers of a step right before they are used, never to the model in memory.
template <bool BACKWARD, bool FORWARD, bool VALUE, bool EXACT, bool BF3, bool MASKED>
__device__ __forceinline__ void tvlqr_mfma16x8_body(const TvLqrArgs &a)
{
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const int i = lane & 15, q = lane >> 4;
    const int T = a.T;
    const int n = EXACT ? N : a.n, m = EXACT ? M : a.m, d = n + m;
    auto zmap = [&](int zi) { return zi < N ? (zi < n ? zi : -1) : (zi - N < m ? n + zi - N : -1); };
    auto Czz = [&](const float *Cg, int zr, int zc) {
        const int r = zmap(zr), c_ = zmap(zc);
        return (r >= 0 && c_ >= 0) ? Cg[r * d + c_] : 0.0f;
    };
    auto cz = [&](const float *cg, int zr) { const int r = zmap(zr); return r >= 0 ? cg[r] : 0.0f; };
    auto Fg_at = [&](int t) { return tv_at(a.F, a.sF_b, a.sF_t, b, t); };
    auto fg_at = [&](int t) { return tv_at(a.f, a.sf_b, a.sf_t, b, t); };
    auto Cg_at = [&](int t) { return tv_at(a.C, a.sC_b, a.sC_t, b, t); };
    auto cg_at = [&](int t) { return tv_at(a.c, a.sc_b, a.sc_t, b, t); };
    float *Kg = a.K + (size_t)b * a.sK;
    float *kg = a.k + (size_t)b * a.sk;
    int status = 0;

    if (BACKWARD) {
        auto load_ops = [&](int t, StepOps &o) {
            const float *Fg = Fg_at(t), *fg = fg_at(t), *Cg = Cg_at(t), *cg = cg_at(t);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 4 * q + r, ku = N + k;
                if (EXACT) {
                    o.F0[r] = Fg[k * D + i];
                    o.F1[r] = (i < M) ? Fg[k * D + N + i] : ((i == M) ? fg[k] : 0.0f);
                    o.C00[r] = Cg[k * D + i];
                    o.C01t[r] = (k < M) ? Cg[(N + k) * D + i] : ((k == M) ? cg[i] : 0.0f);
                    o.C11[r] = (ku < D) ? ((i < M) ? Cg[ku * D + N + i] : ((i == M) ? cg[ku] : 0.0f)) : 0.0f;
                } else {
                    o.F0[r] = (k < n && i < n) ? Fg[k * d + i] : 0.0f;
                    o.F1[r] = (i < M) ? ((k < n && i < m) ? Fg[k * d + n + i] : 0.0f) : ((i == M && k < n) ? fg[k] : 0.0f);
                    o.C00[r] = Czz(Cg, k, i);
                    o.C01t[r] = (k < M) ? Czz(Cg, N + k, i) : ((k == M) ? cz(cg, i) : 0.0f);
                    float c11 = 0.0f;
                    if (ku < D) {
                        if (i < M) c11 = (k >= m && i == k) ? 1.0f : Czz(Cg, ku, N + i);   // unit diagonal on padded actions
                        else if (i == M) c11 = cz(cg, ku);
                    }
                    o.C11[r] = c11;
                }
            }
        };
        // each operand slot has a fixed (row, column): a held control i clears this lane's F1 (column i), a held control
        // k = 4q + r its C01t[r] (row k), and either leaves C11[r] the unit matrix's entry; w is uniform over the wave
        auto mask_ops = [&](uint32_t w, StepOps &o) {
            const bool ci = i < M && (w >> i & 1u);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 4 * q + r;
                const bool ck = k < M && (w >> k & 1u);
                o.F1[r] = ci ? 0.0f : o.F1[r];
                o.C01t[r] = ck ? 0.0f : o.C01t[r];
                o.C11[r] = (k < M && (ci || ck)) ? ((i == k) ? 1.0f : 0.0f) : o.C11[r];
            }
        };
        const uint32_t *mg = MASKED ? a.mask + (size_t)b * T : nullptr;
        uint32_t wcur = MASKED ? mg[T - 1] : 0u, wnxt = 0u;
        StepOps cur, nxt;
        load_ops(T - 1, cur);
        // terminal value function: the final cost, or C_{T-1}[:n,:n], c_{T-1}[:n]; v lives in lanes i == 8
        f32x4 Vd, vd;
        if (a.Cfin) {
            const float *Cf = a.Cfin + (size_t)b * a.sCfin_b, *cf = a.cfin + (size_t)b * a.scfin_b;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 4 * q + r;
                Vd[r] = (EXACT || (k < n && i < n)) ? Cf[k * n + i] : 0.0f;
                vd[r] = (i == M && (EXACT || k < n)) ? cf[k] : 0.0f;
            }
        } else {
            const float *cg = cg_at(T - 1);
            Vd = cur.C00;
#pragma unroll
            for (int r = 0; r < 4; ++r) vd[r] = (i == M && (EXACT || 4 * q + r < n)) ? cg[4 * q + r] : 0.0f;
        }
        float cst = 0.0f;
        int min_pivot_bits = 0x3f800000;
        for (int idx = lane; idx < kZs; idx += kWave) lds[idx] = 0.0f;   // pad columns stay 0
        constexpr int kZero = kMs + 25 * 8;
        constexpr int kQx = kMs + 28 * 8;
        const int t01_src = (i == M) ? kQx + 4 * q : kZero;
        const int g1_src = (i == M) ? kKs + (N + M) * 8 + q : kZero + q;
        __syncthreads();

        for (int t = T - 1; t >= 0; --t) {
            // step t-1's operands in flight while step t computes (clamped: unconditional, see the rollout ring)
            load_ops(t > 0 ? t - 1 : 0, nxt);
            if (MASKED) {
                wnxt = mg[t > 0 ? t - 1 : 0];
                mask_ops(wcur, cur);
            }
            ConstFrag Fc0{}, Fc1{};
            if (BF3) {
                Fc0 = const_frag(f32x4{cur.F0[0], cur.F0[1], cur.F0[2], cur.F0[3]});
                Fc1 = const_frag(f32x4{cur.F1[0], cur.F1[1], cur.F1[2], cur.F1[3]});
            }
            // 1. W = V F~_t (+ v on column 24)
            f32x4 W0 = {0.f, 0.f, 0.f, 0.f}, W1 = {0.f, 0.f, 0.f, 0.f};
            if (BF3) {
                const VarFrag Vf = var_frag(Vd);
                W0 = mm_var_const(Vf, Fc0, W0);
                W1 = mm_var_const(Vf, Fc1, W1);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    W0 = mfma(Vd[r], cur.F0[r], W0);
                    W1 = mfma(Vd[r], cur.F1[r], W1);
                }
            }
            float fw = 0.0f, fv = 0.0f;
            if (VALUE) {     // f_t^T (V f_t) and f_t^T v for the const recursion
                float pw = 0.0f, pv = 0.0f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pw = fmaf(cur.F1[r], W1[r], pw);
                    pv = fmaf(cur.F1[r], vd[r], pv);
                }
                fw = wave_sum(i == M ? pw : 0.0f);
                fv = wave_sum(i == M ? pv : 0.0f);
            }
            W1 += vd;
            // 2. Q~ = C~_t + F~_t^T W: Q_xx, [Q_uu | q_u], and W_1^T F_x (rows 0..7 Q_ux, row 8 q_x^T)
            f32x4 T00 = cur.C00, T01t = cur.C01t, T11 = cur.C11;
            if (BF3) {
                const VarFrag W0f = var_frag(W0), W1f = var_frag(W1);
                T00 = mm_const_var(Fc0, W0f, T00);
                T01t = mm_var_const(W1f, Fc0, T01t);
                T11 = mm_const_var(Fc1, W1f, T11);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    T00 = mfma(cur.F0[r], W0[r], T00);
                    T01t = mfma(W1[r], cur.F0[r], T01t);
                    T11 = mfma(cur.F1[r], W1[r], T11);
                }
            }
            // 3. [Q_ux | Q_uu | q_u] -> column-per-lane layout through LDS
            if (q < 2) {
                *reinterpret_cast<f32x4 *>(&lds[kMs + i * 8 + 4 * q]) = T01t;
                if (i <= M) *reinterpret_cast<f32x4 *>(&lds[kMs + (N + i) * 8 + 4 * q]) = T11;
            } else if (q == 2) {
                lds[kQx + i] = T01t[0];
            }
            lds_sync();
            f32x2 M2[4];
            {
                const int c = lane & 31;
                const f32x4 lo = *reinterpret_cast<const f32x4 *>(&lds[kMs + c * 8]);
                const f32x4 hi = *reinterpret_cast<const f32x4 *>(&lds[kMs + c * 8 + 4]);
                M2[0] = f32x2{lo[0], lo[1]}; M2[1] = f32x2{lo[2], lo[3]};
                M2[2] = f32x2{hi[0], hi[1]}; M2[3] = f32x2{hi[2], hi[3]};
            }
            float quk = 0.0f;
            float qu_saved[8];
            if (VALUE) {
#pragma unroll
                for (int p = 0; p < 8; ++p) qu_saved[p] = readlane(M2[p >> 1][p & 1], 24);
            }
            float Mr[8];
            ldlt8_solve_neg(M2, Mr, min_pivot_bits);
            if (VALUE) {
#pragma unroll
                for (int p = 0; p < 8; ++p) quk = fmaf(readlane(Mr[p], 24), qu_saved[p], quk);
            }
            if (lane < 32) {
                f32x4 lo, hi;
#pragma unroll
                for (int r = 0; r < 4; ++r) { lo[r] = Mr[r]; hi[r] = Mr[4 + r]; }
                *reinterpret_cast<f32x4 *>(&lds[kKs + lane * 8]) = lo;
                *reinterpret_cast<f32x4 *>(&lds[kKs + lane * 8 + 4]) = hi;
            }
            lds_sync();
            // 4. V' = Q_xx + Q_xu K ; v' = q_x + Q_xu k
            f32x4 vacc = *reinterpret_cast<const f32x4 *>(&lds[t01_src]);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const float ax = lds[kMs + i * 8 + 4 * s2 + q];
                const float g0 = lds[kKs + i * 8 + 4 * s2 + q];
                const float g1 = lds[g1_src + 4 * s2];
                T00 = mfma(ax, g0, T00);
                vacc = mfma(ax, g1, vacc);
            }
            {   // V' <- (V' + V'^T) / 2
                float *vt = &lds[kZs];
                *reinterpret_cast<f32x4 *>(&vt[i * kVtLd + 4 * q]) = T00;
                lds_sync();
#pragma unroll
                for (int r = 0; r < 4; ++r) Vd[r] = 0.5f * (T00[r] + vt[(4 * q + r) * kVtLd + i]);
            }
            vd = vacc;
            {   // gains to HBM, row-major K[t][a][j], k[t][a]
                const int ka = lane >> 3, jc = lane & 7;
                float2 kv;
                kv.x = lds[kKs + (2 * jc) * 8 + ka];
                kv.y = lds[kKs + (2 * jc + 1) * 8 + ka];
                if (EXACT) {
                    *reinterpret_cast<float2 *>(&Kg[(size_t)t * (M * N) + 2 * lane]) = kv;
                    if (lane < M) kg[(size_t)t * M + lane] = lds[kKs + 24 * 8 + lane];
                } else {
                    if (ka < m && 2 * jc < n) Kg[(size_t)t * m * n + ka * n + 2 * jc] = kv.x;
                    if (ka < m && 2 * jc + 1 < n) Kg[(size_t)t * m * n + ka * n + 2 * jc + 1] = kv.y;
                    if (lane < m) kg[(size_t)t * m + lane] = lds[kKs + 24 * 8 + lane];
                }
            }
            if (VALUE) {
                // const += 1/2 k^T Q_uu k + k^T q_u + 1/2 f_t^T V f_t + f_t^T v with Q_uu k = -q_u
                cst += 0.5f * quk + 0.5f * fw + fv;
                if (a.V) {
                    float *Vo = a.V + ((size_t)b * T + t) * (n * n);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (EXACT || (4 * q + r < n && i < n)) Vo[(4 * q + r) * n + i] = Vd[r];
                }
                if (a.v && i == M) {
                    float *vo = a.v + ((size_t)b * T + t) * n;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (EXACT || 4 * q + r < n) vo[4 * q + r] = vd[r];
                }
                if (a.cst && lane == 0) a.cst[(size_t)b * T + t] = cst;
            }
            lds_sync();
            cur = nxt;
            if (MASKED) wcur = wnxt;
        }
        if (min_pivot_bits <= 0) status |= (min_pivot_bits == 0) ? TFMPC_ST_SINGULAR : TFMPC_ST_NOT_PD;
        if (VALUE && !(cst == cst)) status |= TFMPC_ST_NAN;
    }

    if (FORWARD) {
        const int fi = lane >> 2, fc = lane & 3;       // F_t: row fi, columns 6fc..6fc+5 (z index)
        const int ka = lane >> 3, jc = lane & 7;       // K_t: row ka, columns 2jc, 2jc+1
        float *xs = a.states + (size_t)b * (T + 1) * n;
        float *us = a.actions + (size_t)b * T * m;
        float *cs = a.costs + (size_t)b * (T + 1);
        float *zs = &lds[kZs];
        __syncthreads();                               // gains written above are visible
        if (lane < N) {
            const float x = (EXACT || lane < n) ? a.x0[(size_t)b * n + lane] : 0.0f;
            zs[lane] = x;
            if (EXACT || lane < n) xs[lane] = x;
        }
        struct Slot { float2 K; float k; float F[6]; float f; };
        auto load_slot = [&](int t, Slot &s) {
            const float *Fg = Fg_at(t);
            if (EXACT) {
                s.K = *reinterpret_cast<const float2 *>(&Kg[(size_t)t * (M * N) + 2 * lane]);
                s.k = kg[(size_t)t * M + ka];
                const float2 *p = reinterpret_cast<const float2 *>(Fg + fi * D + 6 * fc);
#pragma unroll
                for (int j = 0; j < 3; ++j) { const float2 v = p[j]; s.F[2 * j] = v.x; s.F[2 * j + 1] = v.y; }
            } else {
                const bool row = ka < m;
                s.K.x = (row && 2 * jc < n) ? Kg[(size_t)t * m * n + ka * n + 2 * jc] : 0.0f;
                s.K.y = (row && 2 * jc + 1 < n) ? Kg[(size_t)t * m * n + ka * n + 2 * jc + 1] : 0.0f;
                s.k = row ? kg[(size_t)t * m + ka] : 0.0f;
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const int zc = 6 * fc + j;
                    const int col = zc < N ? (zc < n ? zc : -1) : (zc - N < m ? n + zc - N : -1);
                    s.F[j] = (fi < n && col >= 0) ? Fg[fi * d + col] : 0.0f;
                }
            }
            s.f = (fc == 0 && (EXACT || fi < n)) ? fg_at(t)[fi] : 0.0f;      // f enters one of the four partial sums
        };
        Slot R[kRing];
#pragma unroll
        for (int s = 0; s < kRing; ++s) load_slot(s < T ? s : T - 1, R[s]);
        __syncthreads();

        // stage costs of rows [0, rows) of the chunk buffer, step t0 + row: 1/2 z^T C_t z + c_t^T z, one wave-wide sum per
        // step over the d x d entries of C_t (lane e, e + 64, ...), the next step's C_t, c_t in flight
        constexpr int kCe = (D * D + kWave - 1) / kWave;      // entries of C per lane (9)
        int zrc[kCe];                                          // z indices (row | col << 8) of this lane's entries; -1: none
#pragma unroll
        for (int j = 0; j < kCe; ++j) {
            const int e = lane + kWave * j;
            if (e < d * d) {
                const int r = e / d, c_ = e - r * d;
                zrc[j] = (r < n ? r : N + r - n) | ((c_ < n ? c_ : N + c_ - n) << 8);
            } else {
                zrc[j] = -1;
            }
        }
        const int zc1 = lane < d ? (lane < n ? lane : N + lane - n) : -1;
        auto load_cost = [&](int t, float (&Ce)[kCe], float &ce) {
            const float *Cg = Cg_at(t);
#pragma unroll
            for (int j = 0; j < kCe; ++j) Ce[j] = zrc[j] >= 0 ? Cg[lane + kWave * j] : 0.0f;
            ce = zc1 >= 0 ? cg_at(t)[lane] : 0.0f;
        };
        auto chunk_costs = [&](int t0, int rows, float *out) {
            float Ce[kCe], ce, Cn[kCe], cn;
            load_cost(t0, Ce, ce);
            for (int row = 0; row < rows; ++row) {
                load_cost(t0 + (row + 1 < rows ? row + 1 : row), Cn, cn);
                const float *z = zs + row * kZld;
                float part = 0.0f;
#pragma unroll
                for (int j = 0; j < kCe; ++j)
                    if (zrc[j] >= 0) part = fmaf(0.5f * Ce[j], z[zrc[j] & 0xff] * z[zrc[j] >> 8], part);
                if (zc1 >= 0) part = fmaf(ce, z[zc1], part);
                const float s = wave_sum(part);
                if (lane == 0) out[row] = s;
#pragma unroll
                for (int j = 0; j < kCe; ++j) Ce[j] = Cn[j];
                ce = cn;
            }
        };

        for (int t0 = 0; t0 < T; t0 += kTC) {
            const int tc = (T - t0 < kTC) ? (T - t0) : kTC;
            for (int tb = 0; tb < tc; tb += kRing) {
#pragma unroll
                for (int s = 0; s < kRing; ++s) {
                    const int tt = tb + s;
                    if (tt >= tc) break;
                    const int t = t0 + tt;
                    float *zt = zs + tt * kZld;
                    const Slot c = R[s];
                    load_slot(t + kRing < T ? t + kRing : T - 1, R[s]);
                    // u = K_t x + k_t
                    const float2 xv = *reinterpret_cast<const float2 *>(&zt[2 * jc]);
                    float u = fmaf(c.K.x, xv.x, c.K.y * xv.y);
                    u += dpp<kDppXor1>(u);
                    u += dpp<kDppXor2>(u);
                    u += dpp<kDppHalfMirror>(u);
                    u += c.k;
                    zt[N + ka] = u;
                    lds_sync();
                    // x' = F_t z + f_t
                    float xn = c.f;
                    const float2 *zp = reinterpret_cast<const float2 *>(&zt[6 * fc]);
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const float2 z2 = zp[j];
                        xn = fmaf(c.F[2 * j], z2.x, xn);
                        xn = fmaf(c.F[2 * j + 1], z2.y, xn);
                    }
                    xn += dpp<kDppXor1>(xn);
                    xn += dpp<kDppXor2>(xn);
                    zt[kZld + fi] = xn;
                    lds_sync();
                }
            }
            chunk_costs(t0, tc, cs + t0);
            if (EXACT) {
                for (int idx = lane; idx < tc * N; idx += kWave)
                    xs[(size_t)(t0 + 1) * N + idx] = zs[(1 + idx / N) * kZld + (idx & (N - 1))];
                for (int idx = lane; idx < tc * M; idx += kWave)
                    us[(size_t)t0 * M + idx] = zs[(idx / M) * kZld + N + (idx & (M - 1))];
            } else {
                for (int idx = lane; idx < tc * n; idx += kWave)
                    xs[(size_t)(t0 + 1) * n + idx] = zs[(1 + idx / n) * kZld + idx % n];
                for (int idx = lane; idx < tc * m; idx += kWave)
                    us[(size_t)t0 * m + idx] = zs[(idx / m) * kZld + N + idx % m];
            }
            lds_sync();
            if (lane < N) zs[lane] = zs[tc * kZld + lane];      // carry x into row 0 of the next chunk
            lds_sync();
        }
        // final cost 1/2 x^T C_fin x + c_fin^T x (default C_{T-1}[:n,:n], c_{T-1}[:n])
        {
            const float *Cf = a.Cfin ? a.Cfin + (size_t)b * a.sCfin_b : Cg_at(T - 1);
            const float *cf = a.Cfin ? a.cfin + (size_t)b * a.scfin_b : cg_at(T - 1);
            const int ld = a.Cfin ? n : d;
            float part = 0.0f;
            for (int e = lane; e < n * n; e += kWave) {
                const int r = e / n, c_ = e - r * n;
                part = fmaf(0.5f * Cf[r * ld + c_], zs[r] * zs[c_], part);
            }
            if (lane < n) part = fmaf(cf[lane], zs[lane], part);
            const float fcost = wave_sum(part);
            if (lane == 0) cs[T] = fcost;
            if (!(fcost == fcost)) status |= TFMPC_ST_NAN;
        }
    }

    if (a.status && lane == 0) a.status[b] = status;
}

template <bool BACKWARD, bool FORWARD, bool VALUE, bool EXACT, bool BF3>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(TFMPC_TVLQR_EU, TFMPC_TVLQR_EU))) void tvlqr_mfma16x8_kernel(TvLqrArgs a)
{
    tvlqr_mfma16x8_body<BACKWARD, FORWARD, VALUE, EXACT, BF3, false>(a);
}

// The fused solve on a masked model (tvlqr_solve_masked_f32): the adjoint of a control-limited solve.
template <bool EXACT, bool BF3>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(EXACT ? 4 : 3, EXACT ? 4 : 3))) void tvlqr_masked16x8_sweep(TvLqrArgs a)
{
    tvlqr_mfma16x8_body<true, true, false, EXACT, BF3, true>(a);
}

bool use_bf16x3() { return !option_is(kOptLqrMfma, "f32"); }

template <bool BW, bool FW, bool VAL>
int launch(const TvLqrArgs &a, hipStream_t stream)
{
    // EXACT moves F_t rows and gains as float2: every step's F_t and K_t must start on 8 bytes (else the padded path)
    auto even = [](const void *p, long s) { return ((uintptr_t)p & 7) == 0 && (s & 1) == 0; };
    const bool exact = a.n == N && a.m == M && even(a.F, a.sF_b) && even(a.F, a.sF_t) && even(a.K, a.sK);
    const bool bf3 = BW && use_bf16x3();
    const dim3 grid(a.B), block(kWave);
    if (exact && bf3) hipLaunchKernelGGL((tvlqr_mfma16x8_kernel<BW, FW, VAL, true, true>), grid, block, 0, stream, a);
    else if (exact) hipLaunchKernelGGL((tvlqr_mfma16x8_kernel<BW, FW, VAL, true, false>), grid, block, 0, stream, a);
    else if (bf3) hipLaunchKernelGGL((tvlqr_mfma16x8_kernel<BW, FW, VAL, false, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((tvlqr_mfma16x8_kernel<BW, FW, VAL, false, false>), grid, block, 0, stream, a);
    return hipGetLastError() == hipSuccess ? TFMPC_OK : TFMPC_ERR_LAUNCH;
}

int launch_masked(const TvLqrArgs &a, hipStream_t stream)
{
    auto even = [](const void *p, long s) { return ((uintptr_t)p & 7) == 0 && (s & 1) == 0; };
    const bool exact = a.n == N && a.m == M && even(a.F, a.sF_b) && even(a.F, a.sF_t) && even(a.K, a.sK);
    const bool bf3 = use_bf16x3();
    const dim3 grid(a.B), block(kWave);
    if (exact && bf3) hipLaunchKernelGGL((tvlqr_masked16x8_sweep<true, true>), grid, block, 0, stream, a);
    else if (exact) hipLaunchKernelGGL((tvlqr_masked16x8_sweep<true, false>), grid, block, 0, stream, a);
    else if (bf3) hipLaunchKernelGGL((tvlqr_masked16x8_sweep<false, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((tvlqr_masked16x8_sweep<false, false>), grid, block, 0, stream, a);
    return hipGetLastError() == hipSuccess ? TFMPC_OK : TFMPC_ERR_LAUNCH;
}

}  // namespace

bool tvlqr_mfma_supported(int n, int m) { return n >= 1 && m >= 1 && n <= N && m <= M; }

int tvlqr_mfma_launch(const TvLqrArgs &a, bool backward, bool forward, hipStream_t stream)
{
    const bool value = a.V || a.v || a.cst;
    if (a.mask) return (backward && forward && !value) ? launch_masked(a, stream) : TFMPC_ERR_ARG;
    if (backward && forward) return value ? launch<true, true, true>(a, stream) : launch<true, true, false>(a, stream);
    if (backward) return value ? launch<true, false, true>(a, stream) : launch<true, false, false>(a, stream);
    return launch<false, true, false>(a, stream);
}

}  // namespace tfmpc
