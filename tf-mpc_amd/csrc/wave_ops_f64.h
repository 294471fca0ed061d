// wave_ops_f64.h -- what is double-only among the wave-per-instance building blocks: the 64-bit DPP move, the
// wave_sum and finite overloads built on it, and the f64 matrix-core product; then the precision policies (WaveF32,
// WaveF64) of the bodies that serve both precisions.  Everything else (load_matrix,
// wave_gauss_jordan, symmetrise, wave_matvec, wave_for_2d) is wave_ops.h's own template, instantiated with double;
// wave_max(double) is defined there too, ahead of the pivot search that calls it.
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
__device__ __forceinline__ double wave_sum(double v)
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

__device__ __forceinline__ bool finite(double x) { return fabs(x) <= DBL_MAX; }

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

// The precision policies of the bodies that serve fp32 and double (tvlqr_wave.h, tvlqr_box_body.h): the scalar type and
// the matrix-core product, nothing else.  MAXD is the compile-time bound on n and m (16 or 32), i.e. on the k-steps of
// every double product.
struct WaveF32 {
    using T = float;
    template <class FA, class FB, class FInit, class FOut>
    static __device__ __forceinline__ void matmul(int M, int N, int K, FA a, FB b, FInit init, FOut out)
    {
        wave_matmul_mfma(M, N, K, a, b, init, out);
    }
};

template <int MAXD>
struct WaveF64 {
    using T = double;
    template <class FA, class FB, class FInit, class FOut>
    static __device__ __forceinline__ void matmul(int M, int N, int K, FA a, FB b, FInit init, FOut out)
    {
        wave_matmul_f64<MAXD>(M, N, K, a, b, init, out);
    }
};

// which of the two instantiations (MAXD = 16 or 32) serves a shape
inline bool wave16(int n, int m) { return n <= 16 && m <= 16; }

}  // namespace tfmpc
