// wave_ops_f64.h -- the double-precision twins of the wave-per-instance building blocks of wave_ops.h, for
// tvlqr_f64.hip.  Separate functions, not templates of the fp32 ones: the fp32 kernels' code does not change.
//
// Matrix products run on v_mfma_f64_16x16x4_f64.  Its operands are one double per lane, A[l & 15][k = l >> 4] and
// B[k = l >> 4][l & 15] as the f32 16x16x4 form, but its C/D map is NOT the f32 one: register r of lane l holds
// column l & 15 of row (l >> 4) + 4 r (the f32 form: row 4 (l >> 4) + r).
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>

#include "wave_ops.h"

namespace tfmpc {

// A 64-bit cross-lane move: the DPP path moves 32 bits, so the two halves of the double travel separately.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ double dpp_move_f64(double v)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, ROW_MASK, 0xF, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, ROW_MASK, 0xF, false);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// wave_sum of wave_ops.h in double: the same butterfly, the same order of additions; lanes outside a row mask add +0.0
__device__ __forceinline__ double wave_sum_f64(double v)
{
    v += dpp_move_f64<kDppQuadXor1>(v);
    v += dpp_move_f64<kDppQuadXor2>(v);
    v += dpp_move_f64<kDppRowHalfMirror>(v);
    v += dpp_move_f64<kDppRowMirror>(v);
    v += dpp_move_f64<kDppRowBcast15, 0xA>(v);
    v += dpp_move_f64<kDppRowBcast31, 0xC>(v);
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), 63);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ bool finite_f64(double x) { return fabs(x) <= DBL_MAX; }

// out(i, j, init(i, j) + sum_k a(i, k) b(k, j)), i < M, j < N, in 16 x 16 output tiles on v_mfma_f64_16x16x4_f64, one
// wave.  Rows, columns and k beyond the matrix are ZERO operands (the read itself is clamped into the matrix, so no
// address leaves it); their products land in outputs that are not stored.  K <= KMAX (a multiple of 4): the k-steps
// are unrolled and the ones past K skipped, the same sequence of accumulations for every KMAX.
template <int KMAX, class FA, class FB, class FInit, class FOut>
__device__ __forceinline__ void wave_matmul_f64(int M, int N, int K, FA a, FB b, FInit init, FOut out)
{
    using f64x4 = __attribute__((ext_vector_type(4))) double;
    static_assert(KMAX % 4 == 0, "whole k-steps");
    const int lane = lane_id(), li = lane & 15, lq = lane >> 4;
    const int rt = (M + 15) >> 4, ct = (N + 15) >> 4;
    for (int ti = 0; ti < rt; ++ti) {
        const int i0 = 16 * ti;
        const bool ain = i0 + li < M;
        const int ia = ain ? i0 + li : M - 1;
        for (int tj = 0; tj < ct; ++tj) {
            const int j0 = 16 * tj;
            const bool bin = j0 + li < N;
            const int jb = bin ? j0 + li : N - 1;
            f64x4 acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + lq + 4 * r;
                const double x = init(row < M ? row : M - 1, jb);
                acc[r] = (row < M && bin) ? x : 0.0;
            }
#pragma unroll
            for (int s = 0; s < KMAX / 4; ++s) {
                if (4 * s < K) {
                    const bool kin = 4 * s + lq < K;
                    const int kc = kin ? 4 * s + lq : K - 1;
                    double av = a(ia, kc), bv = b(kc, jb);
                    av = (ain && kin) ? av : 0.0;
                    bv = (bin && kin) ? bv : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + lq + 4 * r;
                if (row < M && bin) out(row, j0 + li, acc[r]);
            }
        }
    }
}

// Global -> LDS copy of a row-major [rows][cols] matrix of doubles into leading dimension ld.
__device__ __forceinline__ void load_matrix_f64(double *dst, int ld, const double *src, int rows, int cols)
{
    wave_for_2d(rows, cols, [&](int r, int c, int idx) { dst[r * ld + c] = src[idx]; });
}

// wave_gauss_jordan<false> of wave_ops.h in double: in-place elimination WITHOUT pivoting of aug[rows][width]
// (leading dimension ld), whose first `rows` columns hold a symmetric matrix; on return columns rows .. width - 1 hold
// A^-1 RHS.  A column per lane; fac[rows] is LDS scratch.  Returns 1 if a pivot was non-positive or NaN (the matrix
// is not positive definite), else 0; all lanes return the same value.
__device__ __forceinline__ int wave_eliminate_f64(double *aug, int ld, int rows, int width, double *fac)
{
    const int lane = lane_id();
    int bad = 0;
    for (int p = 0; p < rows; ++p) {
        for (int i = lane; i < rows; i += kWave) fac[i] = aug[i * ld + p];
        wsync();
        const double pv = fac[p];
        if (!(pv > 0.0)) bad = 1;
        const double inv = 1.0 / pv;
        for (int j = lane; j < width; j += kWave) {
            const double pr = aug[p * ld + j] * inv;
            for (int i = 0; i < rows; ++i) {
                const double old = aug[i * ld + j];
                aug[i * ld + j] = (i == p) ? pr : fma(-fac[i], pr, old);
            }
        }
        wsync();
    }
    return bad;
}

}  // namespace tfmpc
