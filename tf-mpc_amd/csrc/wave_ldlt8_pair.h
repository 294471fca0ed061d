// wave_ldlt8_pair.h -- the 8 x 8 SPD solve of wave_ldlt8.h for TWO independent systems in one wave (lqr_mfma16x8.hip, paired launches).
// Layout ("one column per lane, eight rows in registers", as there), by rows of 16 lanes:
//   lanes  0..31: system A,  lanes 32..63: system B;  each system owns two rows of 16 lanes, and in EACH of them
//   lanes 0..7 of the row: columns 0..7 of Q_uu (every row carries its own copy);  lanes 8..15: eight payload columns.
// The payload is 17 columns (16 of Q_ux plus q_u): the elimination reads only the upper triangle of Q_uu, so the lane of Q_uu column 0
// is read for pivot 0 and never again -- the SECOND row of each system keeps q_u there, and every lane takes d_0 = Q_uu[0][0] from the
// caller (it is an input: a broadcast LDS read ahead of the pivot chain).
#pragma once

#include <hip/hip_runtime.h>

#include <utility>

#include "wave_ldlt8.h"      // f32x2, and the solve this one restates

namespace tfmpc {

// Lane L of each row of 16 lanes, given to the whole row (DPP row_newbcast:L, gfx90a+) as the first source of the instruction that uses it:
// v_rcp_f32 for the pivots, v_fmac_f32 for the multipliers, v_min_i32 for the status.  No LDS traffic, no scalar register and no separate
// move: the value is per ROW, which is what lets two systems share a wave.
// Written as instructions because the compiler keeps `v_mov_b32_dpp` + `v_fma_f32` apart (63 moves per solve).  It does not look for hazards
// inside them, so each carries its own wait states: two ahead of a DPP read of a register a vector instruction has just written, one behind
// the transcendental v_rcp_f32.  (s_nop delays this wave alone; the SIMD issues from the others.)
template <int L>
__device__ __forceinline__ float rcp_neg_row_bcast(float v)          // rcp(-v[lane L of the row])
{
    static_assert(L >= 0 && L < 16, "a row has 16 lanes");
    float r;
    asm("s_nop 1\n\tv_rcp_f32_dpp %0, -%1 row_newbcast:%2 row_mask:0xf bank_mask:0xf\n\ts_nop 0" : "=v"(r) : "v"(v), "n"(L));
    return r;
}
template <int L>
__device__ __forceinline__ int min_row_bcast(int v, int m)            // min(v[lane L of the row], m)
{
    static_assert(L >= 0 && L < 16, "a row has 16 lanes");
    asm("s_nop 1\n\tv_min_i32_dpp %0, %1, %0 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(m) : "v"(v), "n"(L));
    return m;
}
template <int L>
__device__ __forceinline__ float fma_row_bcast(float v, float b, float acc)    // fmaf(v[lane L of the row], b, acc)
{
    static_assert(L >= 0 && L < 16, "a row has 16 lanes");
    asm("s_nop 1\n\tv_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(v), "v"(b), "n"(L));
    return acc;
}

namespace ldlt8_pair_detail {
template <class F, int... I>
__device__ __forceinline__ void static_for(F &&f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
}  // namespace ldlt8_pair_detail

// ldlt8_solve_neg (wave_ldlt8.h) with the multipliers per row of 16 lanes.  Every element goes through EXACTLY the chain of fused
// multiply-adds it goes through there -- the same multiplier, the same operands in the same order, the same rcp(-d) -- so every column comes
// out bit-identical to the single-system solve, whatever rides in the other rows.  Two things differ in form only: the updates are single
// v_fmac_f32 (the broadcast is their first source; v_pk_fma_f32 is two such IEEE FMAs and takes no DPP source), and the back substitution runs
// row by row (the updates of one element keep their order s = 7 .. p+1; rows do not depend on rows below them).
//   d0              Q_uu[0][0] of the lane's system (all lanes)
//   min_pivot_bits  PER LANE: the smallest pivot seen by the lane's row, as float bits (v_min_i32); the rows of one system agree, those of
//                   different systems never mix
__device__ __forceinline__ void ldlt8_pair_solve_neg(f32x2 (&M2)[4], float (&X)[8], float d0, int &min_pivot_bits)
{
    using namespace ldlt8_pair_detail;
    f32x2 N2[4];
    // forward: every multiplier -L[s][p] = (-row_p / d_p)[column s] is used by ONE update, right where it is broadcast
    static_for([&](auto P) {
        constexpr int p = decltype(P)::value;
        constexpr int pp = p >> 1, ps = p & 1;
        const float Mp = M2[pp][ps];
        float ninv;
        if constexpr (p == 0) {
            const int pvb = __builtin_bit_cast(int, d0);
            min_pivot_bits = pvb < min_pivot_bits ? pvb : min_pivot_bits;
            ninv = __builtin_amdgcn_rcpf(-d0);
        } else {
            min_pivot_bits = min_row_bcast<p>(__builtin_bit_cast(int, Mp), min_pivot_bits);
            ninv = rcp_neg_row_bcast<p>(Mp);
        }
        const float Mn = Mp * ninv;                      // -row_p / d_p
        N2[pp][ps] = Mn;
        static_for([&](auto S) {
            constexpr int s = p + 1 + decltype(S)::value;
            M2[s >> 1][s & 1] = fma_row_bcast<s>(Mn, Mp, M2[s >> 1][s & 1]);
        }, std::make_integer_sequence<int, 7 - p>{});
    }, std::make_integer_sequence<int, 8>{});
    // backward, row by row: X_p = N_p + sum_{s = 7 .. p+1} (-L[s][p]) X_s.  Row p's multipliers still sit in its own Q_uu lanes when its turn
    // comes (only row p's updates change them), so they are broadcast again from a copy of the row, taken before the row is updated,
    // instead of being kept from the forward sweep (28 registers: they were scalars in the one-system solve).
    static_for([&](auto PP) {
        constexpr int p = 6 - decltype(PP)::value;
        const float O = N2[p >> 1][p & 1];
        static_for([&](auto S) {
            constexpr int s = 7 - decltype(S)::value;
            N2[p >> 1][p & 1] = fma_row_bcast<s>(O, N2[s >> 1][s & 1], N2[p >> 1][p & 1]);
        }, std::make_integer_sequence<int, 7 - p>{});
    }, std::make_integer_sequence<int, 7>{});
#pragma unroll
    for (int r = 0; r < 8; ++r) X[r] = N2[r >> 1][r & 1];
}

}  // namespace tfmpc
