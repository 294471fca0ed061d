// wave_ldlt8_pair.h -- the 8 x 8 SPD solve of wave_ldlt8.h for TWO independent systems in one wave (lqr_mfma16x8.hip, paired launches).
// Layout ("one column per lane, eight rows in registers", as there), by rows of 16 lanes:
//   lanes  0..31: system A,  lanes 32..63: system B;  each system owns two rows of 16 lanes, and in EACH of them
//   lane 0 of the row: q_u;  lanes 1..7: columns 1..7 of Q_uu (every row carries its own copy);  lanes 8..15: eight columns of Q_ux.
// The payload is 17 columns (16 of Q_ux plus q_u): the elimination reads only the upper triangle of Q_uu, and lane 0 of a row is never a
// broadcast source (pivot 0 takes d_0 = Q_uu[0][0] from the caller -- it is an input: a broadcast LDS read ahead of the pivot chain -- and
// every row_newbcast of the solve names a lane >= 1), so a copy of Q_uu column 0 there would be dead weight: lane 0 of BOTH rows keeps
// q_u instead.  Behind the back substitution lane 0 of every row therefore holds k = -Q_uu^-1 q_u in X[0..7], and lanes 8..15 hold the
// columns of K next to it: the value update v'[j] = q_x[j] + sum_a k[a] Q_ux[a][j] of the sweep is finished right here, in the lane
// of column j, as eight v_fmac_f32 whose first source is lane 0's X[a] (the chain at the end of the statement).
#pragma once

#include <hip/hip_runtime.h>

#include "wave_ldlt8.h"      // f32x2, and the solve this one restates

namespace tfmpc {

// Lane L of each row of 16 lanes, given to the whole row (DPP row_newbcast:L, gfx90a+) as the first source of the instruction that uses it:
// v_rcp_f32 for the pivots, v_fmac_f32 for the multipliers, v_min_i32 for the status.  No LDS traffic, no scalar register and no separate
// move: the value is per ROW, which is what lets two systems share a wave.
// Written as instructions because the compiler keeps `v_mov_b32_dpp` + `v_fma_f32` apart (63 moves per solve), and as ONE asm statement for
// the whole solve because the compiler does not look for hazards inside asm statements and answers with an `s_nop 0` of its own wherever one
// statement hands a register to the next, or to an instruction of its own (20 per solve when every group of broadcasts was a statement, 15
// with one statement per pivot: 7 between the pivots, 7 between the back-substitution rows, 1 between the two).  Inside the statement the order is the written one, so the wait states are counted here, by hand, and
// most of them are instructions the solve needs anyway.  (s_nop delays this wave alone -- but this wave is the one its partner waits for at
// the barrier.)  Two rules: a DPP read needs TWO instructions or wait states between it and the vector instruction that wrote the register;
// a plain instruction that reads the result of the transcendental v_rcp_f32 needs ONE.
//
// Write -> DPP-read pairs of the statement, in program order (m_s: row s of the input, x_s: row s of the result, first -L then X):
//   (a) pivot p >= 1 reads m_p by DPP (v_rcp_f32_dpp, then v_min_i32_dpp).  m_p was last written by the FIRST update of pivot p-1's group
//       and the group's other 7-p updates lie between: two or more for p <= 5; one at p = 6, which takes an `s_nop 0`; none at p = 7, where
//       the two copies the back substitution needs first (rows 5 and 4, below) stand in the gap.
//   (b) every pivot p <= 6: x_p = m_p * ninv (v_mul_f32) and the first v_fmac_f32_dpp of its group reads x_p next: `s_nop 1`.  Pivot 7 has
//       no group; x_7 is only ever a plain operand.
//   (c) every back-substitution row p <= 5 broadcasts the row AS IT WAS before its first update, from a copy.  The copies alternate between
//       the registers of m_0 and m_1 (dead since pivots 0 and 1) and each is made one row early -- behind the last read of the register's
//       previous copy -- so that the 7-p-1 >= 2 updates of the row above lie between copy and first read (rows 5 and 4: all of pivot 7).
//       Row 6 has one update and broadcasts itself: x_6 was written by pivot 6's v_mul_f32, with pivot 6's update and pivot 7 behind it.
//   (d) v_rcp_f32_dpp -> v_mul_f32 (transcendental result read by a plain instruction): the v_min_i32(_dpp) of the pivot stands between.
//   (e) the value chain reads x_0 .. x_7 of lane 0 by DPP, a = 0 first.  x_0 is the LAST row the back substitution writes (its update by
//       x_1 is the instruction ahead of the chain): `s_nop 1`.  x_1 was last written seven instructions earlier, the others earlier still.
// Nothing else: inside a group the broadcast register is only read, every update writes a row of its own (forward) or chains through the
// accumulator (backward: an ordinary interlocked dependence), v_min_i32_dpp's result is read as a plain operand, and the rows x_s a
// back-substitution row multiplies by are plain operands too; the value chain runs through its accumulator and its second sources are inputs
// of the statement.  8 `s_nop 1` and 1 `s_nop 0` in all, none added by the compiler.
#define TFMPC_BC(L) " row_newbcast:" #L " row_mask:0xf bank_mask:0xf\n\t"
// pivot p >= 1: ninv = rcp(-d_p) and the smallest pivot, d_p = lane p of the row's own m_p; x_p = m_p * ninv = -row_p / d_p
#define TFMPC_PIVOT(P) "v_rcp_f32_dpp %[x" #P "], -%[m" #P "]" TFMPC_BC(P) \
                       "v_min_i32_dpp %[mp], %[m" #P "], %[mp]" TFMPC_BC(P) \
                       "v_mul_f32 %[x" #P "], %[m" #P "], %[x" #P "]\n\t"
// forward update of pivot p: m_s = fmaf(x_p[lane s of the row], m_p, m_s)
#define TFMPC_FWD(P, S) "v_fmac_f32_dpp %[m" #S "], %[x" #P "], %[m" #P "]" TFMPC_BC(S)
// back-substitution update of row p: x_p = fmaf(O[lane s of the row], x_s, x_p), O the copy of the row in the register of m_0 or m_1
#define TFMPC_BWD(P, O, S) "v_fmac_f32_dpp %[x" #P "], %[" #O "], %[x" #S "]" TFMPC_BC(S)
#define TFMPC_COPY(O, P) "v_mov_b32 %[" #O "], %[x" #P "]\n\t"
// value chain, term a: acc = fmaf(x_a[lane 0 of the row] (= k[a]), q_a, acc), q_a = row a of the lane's column AS IT CAME IN
#define TFMPC_VAL(A) "v_fmac_f32_dpp %[acc], %[x" #A "], %[q" #A "]" TFMPC_BC(0)

// ldlt8_solve_neg (wave_ldlt8.h) with the multipliers per row of 16 lanes.  Every element goes through EXACTLY the chain of fused
// multiply-adds it goes through there -- the same multiplier, the same operands in the same order, the same rcp(-d) -- so every column comes
// out bit-identical to the single-system solve, whatever rides in the other rows.  Two things differ in form only: the updates are single
// v_fmac_f32 (the broadcast is their first source; v_pk_fma_f32 is two such IEEE FMAs and takes no DPP source), and the back substitution runs
// row by row (the updates of one element keep their order s = 7 .. p+1; rows do not depend on rows below them).
//   forward: every multiplier -L[s][p] = (-row_p / d_p)[column s] is used by ONE update, right where it is broadcast
//   backward, row by row: X_p = N_p + sum_{s = 7 .. p+1} (-L[s][p]) X_s.  Row p's multipliers still sit in its own Q_uu lanes when its turn
//   comes (only row p's updates change them), so they are broadcast again from a copy of the row, taken before the row is updated,
//   instead of being kept from the forward sweep (28 registers: they were scalars in the one-system solve).
//   d0              Q_uu[0][0] of the lane's system (all lanes): pivot 0 takes it from here and uses no broadcast
//   min_pivot_bits  PER LANE: the smallest pivot seen by the lane's row, as float bits (v_min_i32); the rows of one system agree, those of
//                   different systems never mix
//   Q, acc          the value chain: acc = fmaf(k[a], Q[a], acc) for a = 0 .. 7 IN THAT ORDER, k = X[0..7] of lane 0 of the lane's row.  Q is the
//                   lane's column once more (the solve overwrites M2's copy; registers of their own), acc comes in as q_x[j] in the lane of
//                   Q_ux column j and goes out as v'[j].  This is the chain of the one-wave blocks (lqr_mfma16x8.hip), term for term.
//                   (The chain as a statement of its own, which moves the wait for Q's LDS reads behind the solve, costs four register moves
//                   and was not faster: profiles/r12_mfma16x8_budget.md.)
__device__ __forceinline__ void ldlt8_pair_solve_neg(const f32x2 (&M2)[4], float (&X)[8], float d0, int &min_pivot_bits, const float (&Q)[8],
                                                     float &acc)
{
    float M[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) M[r] = M2[r >> 1][r & 1];
    asm("v_rcp_f32 %[x0], -%[d0]\n\t"
        "v_min_i32 %[mp], %[d0], %[mp]\n\t"
        "v_mul_f32 %[x0], %[m0], %[x0]\n\t"
        "s_nop 1\n\t"
        TFMPC_FWD(0, 1) TFMPC_FWD(0, 2) TFMPC_FWD(0, 3) TFMPC_FWD(0, 4) TFMPC_FWD(0, 5) TFMPC_FWD(0, 6) TFMPC_FWD(0, 7)
        TFMPC_PIVOT(1) "s_nop 1\n\t"
        TFMPC_FWD(1, 2) TFMPC_FWD(1, 3) TFMPC_FWD(1, 4) TFMPC_FWD(1, 5) TFMPC_FWD(1, 6) TFMPC_FWD(1, 7)
        TFMPC_PIVOT(2) "s_nop 1\n\t"
        TFMPC_FWD(2, 3) TFMPC_FWD(2, 4) TFMPC_FWD(2, 5) TFMPC_FWD(2, 6) TFMPC_FWD(2, 7)
        TFMPC_PIVOT(3) "s_nop 1\n\t"
        TFMPC_FWD(3, 4) TFMPC_FWD(3, 5) TFMPC_FWD(3, 6) TFMPC_FWD(3, 7)
        TFMPC_PIVOT(4) "s_nop 1\n\t"
        TFMPC_FWD(4, 5) TFMPC_FWD(4, 6) TFMPC_FWD(4, 7)
        TFMPC_PIVOT(5) "s_nop 1\n\t"
        TFMPC_FWD(5, 6) TFMPC_FWD(5, 7)
        "s_nop 0\n\t"
        TFMPC_PIVOT(6) "s_nop 1\n\t"
        TFMPC_FWD(6, 7)
        TFMPC_COPY(m0, 5) TFMPC_COPY(m1, 4)
        TFMPC_PIVOT(7)
        "v_fmac_f32_dpp %[x6], %[x6], %[x7]" TFMPC_BC(7)
        TFMPC_BWD(5, m0, 7) TFMPC_BWD(5, m0, 6)
        TFMPC_COPY(m0, 3)
        TFMPC_BWD(4, m1, 7) TFMPC_BWD(4, m1, 6) TFMPC_BWD(4, m1, 5)
        TFMPC_COPY(m1, 2)
        TFMPC_BWD(3, m0, 7) TFMPC_BWD(3, m0, 6) TFMPC_BWD(3, m0, 5) TFMPC_BWD(3, m0, 4)
        TFMPC_COPY(m0, 1)
        TFMPC_BWD(2, m1, 7) TFMPC_BWD(2, m1, 6) TFMPC_BWD(2, m1, 5) TFMPC_BWD(2, m1, 4) TFMPC_BWD(2, m1, 3)
        TFMPC_COPY(m1, 0)
        TFMPC_BWD(1, m0, 7) TFMPC_BWD(1, m0, 6) TFMPC_BWD(1, m0, 5) TFMPC_BWD(1, m0, 4) TFMPC_BWD(1, m0, 3) TFMPC_BWD(1, m0, 2)
        TFMPC_BWD(0, m1, 7) TFMPC_BWD(0, m1, 6) TFMPC_BWD(0, m1, 5) TFMPC_BWD(0, m1, 4) TFMPC_BWD(0, m1, 3) TFMPC_BWD(0, m1, 2) TFMPC_BWD(0, m1, 1)
        "s_nop 1\n\t"
        TFMPC_VAL(0) TFMPC_VAL(1) TFMPC_VAL(2) TFMPC_VAL(3) TFMPC_VAL(4) TFMPC_VAL(5) TFMPC_VAL(6) TFMPC_VAL(7)
        : [x0] "=&v"(X[0]), [x1] "=&v"(X[1]), [x2] "=&v"(X[2]), [x3] "=&v"(X[3]), [x4] "=&v"(X[4]), [x5] "=&v"(X[5]), [x6] "=&v"(X[6]),
          [x7] "=&v"(X[7]), [m0] "+v"(M[0]), [m1] "+v"(M[1]), [m2] "+v"(M[2]), [m3] "+v"(M[3]), [m4] "+v"(M[4]), [m5] "+v"(M[5]),
          [m6] "+v"(M[6]), [m7] "+v"(M[7]), [mp] "+v"(min_pivot_bits), [acc] "+v"(acc)
        : [d0] "v"(d0), [q0] "v"(Q[0]), [q1] "v"(Q[1]), [q2] "v"(Q[2]), [q3] "v"(Q[3]), [q4] "v"(Q[4]), [q5] "v"(Q[5]), [q6] "v"(Q[6]),
          [q7] "v"(Q[7]));
}
#undef TFMPC_VAL
#undef TFMPC_COPY
#undef TFMPC_BWD
#undef TFMPC_FWD
#undef TFMPC_PIVOT
#undef TFMPC_BC

}  // namespace tfmpc
