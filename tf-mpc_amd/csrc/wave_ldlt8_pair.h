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
// inside asm statements and may reorder independent ones, so the wait states are written out: two ahead of a DPP read of a register a vector
// instruction has just written, one behind the transcendental v_rcp_f32.  (s_nop delays this wave alone -- but this wave is the one its
// partner waits for at the barrier, so they are spent once per GROUP of broadcasts from one register, not once per broadcast.)
//
// Write -> DPP-read pairs of the solve that fall inside the two-instruction window, in program order:
//   (a) pivot p >= 1: row p was last written by the FIRST update of pivot p-1's group, 7-p updates lie behind it, and v_min_i32_dpp reads
//       it next -- 0 instructions between at p = 7 (the single update of pivot 6), 1 at p = 6: inside the window.  p <= 5 has two or more
//       updates between, but only while the compiler leaves the statements where they were written.  v_rcp_f32_dpp reads the same row one
//       instruction later.
//   (b) every pivot p <= 6: Mn = row_p * ninv is a compiler-emitted v_mul_f32 and the first v_fmac_f32_dpp of the group reads it next; the
//       second update would still be inside the window, the others are two or more behind.
//   (c) every back-substitution row p <= 5: the copy of the row (v_mov_b32) and the first update, which reads the copy.  Row 6 has one
//       update and needs no copy: its register was written by pivot 6's v_mul_f32, with pivot 6's update and all of pivot 7 behind it.
//   (d) v_rcp_f32_dpp -> v_mul_f32 (transcendental result read by a plain instruction): one wait state.
// Nothing else: inside a group the broadcast register is only read, every update writes a row of its own (forward) or chains through the
// accumulator (backward: an ordinary interlocked dependence), v_min_i32_dpp's result is read as a plain operand, and the rows X_s a
// back-substitution row multiplies by are plain operands too.
// So every statement below opens with `s_nop 1` ahead of its first DPP read (the back-substitution rows: behind their copy), whatever the
// compiler puts in front of it, and a group is ONE statement: 7 (pivots) + 7 (forward groups) + 7 (rows) `s_nop 1` and 7 `s_nop 0`.
#define TFMPC_ROW_BCAST(L) " row_newbcast:" #L " row_mask:0xf bank_mask:0xf\n\t"
template <int L>
__device__ __forceinline__ void pivot_row_bcast(float v, int &m, float &ninv)     // m = min(v[lane L of the row], m), ninv = rcp(-v[lane L])
{
    static_assert(L >= 1 && L < 16, "a row has 16 lanes");
    asm("s_nop 1\n\t"
        "v_min_i32_dpp %0, %2, %0 row_newbcast:%3 row_mask:0xf bank_mask:0xf\n\t"
        "v_rcp_f32_dpp %1, -%2 row_newbcast:%3 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 0"
        : "+v"(m), "=v"(ninv) : "v"(v), "n"(L));
}
// forward group of pivot p: M[s] = fmaf(Mn[lane s of the row], Mp, M[s]), s = p+1 .. 7
#define TFMPC_FWD(S) "v_fmac_f32_dpp %[a" #S "], %[mn], %[mp]" TFMPC_ROW_BCAST(S)
#define TFMPC_FWD_OPS : [mn] "v"(Mn), [mp] "v"(Mp)
template <int P>
__device__ __forceinline__ void fwd_group_row_bcast(float (&M)[8], float Mn, float Mp)
{
    static_assert(P >= 0 && P <= 6, "pivot 7 updates nothing");
    if constexpr (P == 0)
        asm("s_nop 1\n\t" TFMPC_FWD(1) TFMPC_FWD(2) TFMPC_FWD(3) TFMPC_FWD(4) TFMPC_FWD(5) TFMPC_FWD(6) TFMPC_FWD(7)
            : [a1] "+v"(M[1]), [a2] "+v"(M[2]), [a3] "+v"(M[3]), [a4] "+v"(M[4]), [a5] "+v"(M[5]), [a6] "+v"(M[6]), [a7] "+v"(M[7]) TFMPC_FWD_OPS);
    else if constexpr (P == 1)
        asm("s_nop 1\n\t" TFMPC_FWD(2) TFMPC_FWD(3) TFMPC_FWD(4) TFMPC_FWD(5) TFMPC_FWD(6) TFMPC_FWD(7)
            : [a2] "+v"(M[2]), [a3] "+v"(M[3]), [a4] "+v"(M[4]), [a5] "+v"(M[5]), [a6] "+v"(M[6]), [a7] "+v"(M[7]) TFMPC_FWD_OPS);
    else if constexpr (P == 2)
        asm("s_nop 1\n\t" TFMPC_FWD(3) TFMPC_FWD(4) TFMPC_FWD(5) TFMPC_FWD(6) TFMPC_FWD(7)
            : [a3] "+v"(M[3]), [a4] "+v"(M[4]), [a5] "+v"(M[5]), [a6] "+v"(M[6]), [a7] "+v"(M[7]) TFMPC_FWD_OPS);
    else if constexpr (P == 3)
        asm("s_nop 1\n\t" TFMPC_FWD(4) TFMPC_FWD(5) TFMPC_FWD(6) TFMPC_FWD(7)
            : [a4] "+v"(M[4]), [a5] "+v"(M[5]), [a6] "+v"(M[6]), [a7] "+v"(M[7]) TFMPC_FWD_OPS);
    else if constexpr (P == 4)
        asm("s_nop 1\n\t" TFMPC_FWD(5) TFMPC_FWD(6) TFMPC_FWD(7) : [a5] "+v"(M[5]), [a6] "+v"(M[6]), [a7] "+v"(M[7]) TFMPC_FWD_OPS);
    else if constexpr (P == 5)
        asm("s_nop 1\n\t" TFMPC_FWD(6) TFMPC_FWD(7) : [a6] "+v"(M[6]), [a7] "+v"(M[7]) TFMPC_FWD_OPS);
    else
        asm("s_nop 1\n\t" TFMPC_FWD(7) : [a7] "+v"(M[7]) TFMPC_FWD_OPS);
}
// back-substitution row p: X_p = fmaf(O[lane s of the row], X_s, X_p), s = 7 .. p+1, O the row as it was before its first update
#define TFMPC_BWD(S) "v_fmac_f32_dpp %[x], %[o], %[x" #S "]" TFMPC_ROW_BCAST(S)
#define TFMPC_BWD_COPY "v_mov_b32 %[o], %[x]\n\ts_nop 1\n\t"
template <int P>
__device__ __forceinline__ void bwd_row_bcast(float (&X)[8])
{
    static_assert(P >= 0 && P <= 6, "row 7 is its own solution");
    [[maybe_unused]] float O;     // (early clobber: written before the other rows are read)
    if constexpr (P == 6)
        asm("s_nop 1\n\tv_fmac_f32_dpp %[x], %[x], %[x7]" TFMPC_ROW_BCAST(7) : [x] "+v"(X[6]) : [x7] "v"(X[7]));
    else if constexpr (P == 5)
        asm(TFMPC_BWD_COPY TFMPC_BWD(7) TFMPC_BWD(6) : [x] "+v"(X[5]), [o] "=&v"(O) : [x7] "v"(X[7]), [x6] "v"(X[6]));
    else if constexpr (P == 4)
        asm(TFMPC_BWD_COPY TFMPC_BWD(7) TFMPC_BWD(6) TFMPC_BWD(5) : [x] "+v"(X[4]), [o] "=&v"(O) : [x7] "v"(X[7]), [x6] "v"(X[6]), [x5] "v"(X[5]));
    else if constexpr (P == 3)
        asm(TFMPC_BWD_COPY TFMPC_BWD(7) TFMPC_BWD(6) TFMPC_BWD(5) TFMPC_BWD(4)
            : [x] "+v"(X[3]), [o] "=&v"(O) : [x7] "v"(X[7]), [x6] "v"(X[6]), [x5] "v"(X[5]), [x4] "v"(X[4]));
    else if constexpr (P == 2)
        asm(TFMPC_BWD_COPY TFMPC_BWD(7) TFMPC_BWD(6) TFMPC_BWD(5) TFMPC_BWD(4) TFMPC_BWD(3)
            : [x] "+v"(X[2]), [o] "=&v"(O) : [x7] "v"(X[7]), [x6] "v"(X[6]), [x5] "v"(X[5]), [x4] "v"(X[4]), [x3] "v"(X[3]));
    else if constexpr (P == 1)
        asm(TFMPC_BWD_COPY TFMPC_BWD(7) TFMPC_BWD(6) TFMPC_BWD(5) TFMPC_BWD(4) TFMPC_BWD(3) TFMPC_BWD(2)
            : [x] "+v"(X[1]), [o] "=&v"(O) : [x7] "v"(X[7]), [x6] "v"(X[6]), [x5] "v"(X[5]), [x4] "v"(X[4]), [x3] "v"(X[3]), [x2] "v"(X[2]));
    else
        asm(TFMPC_BWD_COPY TFMPC_BWD(7) TFMPC_BWD(6) TFMPC_BWD(5) TFMPC_BWD(4) TFMPC_BWD(3) TFMPC_BWD(2) TFMPC_BWD(1)
            : [x] "+v"(X[0]), [o] "=&v"(O)
            : [x7] "v"(X[7]), [x6] "v"(X[6]), [x5] "v"(X[5]), [x4] "v"(X[4]), [x3] "v"(X[3]), [x2] "v"(X[2]), [x1] "v"(X[1]));
}
#undef TFMPC_BWD_COPY
#undef TFMPC_BWD
#undef TFMPC_FWD_OPS
#undef TFMPC_FWD
#undef TFMPC_ROW_BCAST

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
__device__ __forceinline__ void ldlt8_pair_solve_neg(const f32x2 (&M2)[4], float (&X)[8], float d0, int &min_pivot_bits)
{
    using namespace ldlt8_pair_detail;
    float M[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) M[r] = M2[r >> 1][r & 1];
    // forward: every multiplier -L[s][p] = (-row_p / d_p)[column s] is used by ONE update, right where it is broadcast
    static_for([&](auto P) {
        constexpr int p = decltype(P)::value;
        const float Mp = M[p];
        float ninv;
        if constexpr (p == 0) {
            const int pvb = __builtin_bit_cast(int, d0);
            min_pivot_bits = pvb < min_pivot_bits ? pvb : min_pivot_bits;
            ninv = __builtin_amdgcn_rcpf(-d0);
        } else {
            pivot_row_bcast<p>(Mp, min_pivot_bits, ninv);
        }
        const float Mn = Mp * ninv;                      // -row_p / d_p
        X[p] = Mn;
        if constexpr (p < 7) fwd_group_row_bcast<p>(M, Mn, Mp);
    }, std::make_integer_sequence<int, 8>{});
    // backward, row by row: X_p = N_p + sum_{s = 7 .. p+1} (-L[s][p]) X_s.  Row p's multipliers still sit in its own Q_uu lanes when its turn
    // comes (only row p's updates change them), so they are broadcast again from a copy of the row, taken before the row is updated,
    // instead of being kept from the forward sweep (28 registers: they were scalars in the one-system solve).
    static_for([&](auto PP) { bwd_row_bcast<6 - decltype(PP)::value>(X); }, std::make_integer_sequence<int, 7>{});
}

}  // namespace tfmpc
