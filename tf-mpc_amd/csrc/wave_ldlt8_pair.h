// wave_ldlt8_pair.h -- the 8 x 8 SPD solve of wave_ldlt8.h for TWO independent systems in one wave (lqr_mfma16x8.hip, paired launches).
// Layout ("one column per lane, eight rows in registers", as there), by rows of 16 lanes:
//   lanes  0..31: system A,  lanes 32..63: system B;  each system owns two rows of 16 lanes, and in EACH of them
//   lane 0 of the row: q_u;  lanes 1..7: columns 1..7 of Q_uu (every row carries its own copy);  lanes 8..15: eight columns of Q_ux.
// The payload is 17 columns (16 of Q_ux plus q_u): the elimination reads only the upper triangle of Q_uu, and lane 0 of a row is never a
// broadcast source (pivot 0 takes d_0 = Q_uu[0][0] from the caller -- it is an input: a broadcast LDS read ahead of the pivot chain -- and
// every row_newbcast of the solve names a lane >= 1), so a copy of Q_uu column 0 there would be dead weight: lane 0 of BOTH rows keeps
// q_u instead.  Lane 0 of every row therefore holds the q_u column of x^ = -m^ / d while the elimination runs (k behind the back
// substitution), and lanes 8..15 hold the columns of Q_ux next to it: the value update v'[j] = q_x[j] + sum_a x^_a[q_u] m^_a[j] of the
// sweep is finished right here, in the lane of column j, as eight v_fmac_f32 whose first source is lane 0's X[a] (woven into the elimination).
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
// with one statement per pivot).  Inside the statement the order is the written one, so the wait states are counted here, by hand, and
// most of them are instructions the solve needs anyway.  (s_nop delays this wave alone -- but this wave is the one its partner waits for at
// the barrier.)  Two rules: a DPP read needs TWO instructions or wait states between it and the vector instruction that wrote the register;
// a plain instruction that reads the result of the transcendental v_rcp_f32 needs ONE.
//
// The value chain is taken from the FORWARD elimination (round 13): with m^_a the row a as it stands when it becomes the pivot row and
// x^_a = -m^_a / d_a, v'[j] = q_x[j] + sum_a x^_a[q_u column] m^_a[j] -- in exact arithmetic q_x + Q_xu k, the update written with the
// factors of Q_uu = L D L^T instead of the solved k.  Both factors of term a are live registers of the elimination from pivot a on, so the
// chain needs no second copy of the column, and its terms stand in the wait states the pivots would otherwise spend in `s_nop`.
//
// Write -> DPP-read pairs of the statement, in program order (m_s: row s of the input, x_s: row s of the result, first x^ then X):
//   (a) pivot p >= 1 reads m_p by DPP (v_rcp_f32_dpp, then v_min_i32_dpp).  m_p was last written by the FIRST update of pivot p-1's group
//       and the group's other 7-p updates lie between: two or more for p <= 5; one at p = 6, where term 5 of the value chain stands next to
//       it; none at p = 7, where term 6 and an `s_nop 0` stand in the gap.
//   (b) every pivot p <= 6: x_p = m_p * ninv (v_mul_f32) and the first v_fmac_f32_dpp of its group reads x_p next: two wait states, of which
//       term p-1 of the value chain is one for p = 1 .. 5 (`s_nop 0` for the other); pivots 0 and 6 take an `s_nop 1`.  Pivot 7 has no group.
//   (c) every back-substitution row p <= 5 broadcasts the row AS IT WAS before its first update, from a copy.  The copies alternate between
//       the registers of m_0 and m_1 (dead since terms 0 and 1 of the value chain, behind pivots 1 and 2) and each is made one row early --
//       behind the last read of the register's previous copy -- so that the 7-p-1 >= 2 updates of the row above lie between copy and first
//       read (rows 5 and 4: the other copy and row 6's update, or more).
//       Row 6 has one update and broadcasts itself: x_6 was written by pivot 6's v_mul_f32, with pivot 6's update and pivot 7 behind it.
//   (d) v_rcp_f32_dpp -> v_mul_f32 (transcendental result read by a plain instruction): the v_min_i32(_dpp) of the pivot stands between.
//   (e) term a of the value chain reads x_a of lane 0 by DPP.  Terms 0 .. 5 stand behind pivot a+1 (x_a was written a whole group earlier),
//       term 6 behind pivot 6's `s_nop 1` and update; term 7 follows pivot 7: `s_nop 1`.  The chain's second source m_a is final once
//       pivot a-1's group has run; m_0 and m_1 are overwritten by the copies only behind pivot 7.
// Nothing else: inside a group the broadcast register is only read, every update writes a row of its own (forward) or chains through the
// accumulator (backward, value chain: an ordinary interlocked dependence), v_min_i32_dpp's result is read as a plain operand, and the rows
// x_s a back-substitution row multiplies by are plain operands too.  3 `s_nop 1` and 6 `s_nop 0` in all, none added by the compiler.
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
// value chain, term a: acc = fmaf(x^_a[lane 0 of the row], m^_a, acc)
#define TFMPC_VAL(A) "v_fmac_f32_dpp %[acc], %[x" #A "], %[m" #A "]" TFMPC_BC(0)

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
//   acc             the value chain: acc = fmaf(x^_a[lane 0 of the lane's row], m^_a, acc) for a = 0 .. 7 IN THAT ORDER.  The caller passes 0
//                   and adds what comes out -- (Q_xu k)[j] in the lane of Q_ux column j -- to q_x[j] in ONE rounding: the eight products are
//                   summed among themselves first.  This is the chain of the one-wave blocks (lqr_mfma16x8.hip), term for term.
__device__ __forceinline__ void ldlt8_pair_solve_neg(const f32x2 (&M2)[4], float (&X)[8], float d0, int &min_pivot_bits, float &acc)
{
    float M[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) M[r] = M2[r >> 1][r & 1];
    asm("v_rcp_f32 %[x0], -%[d0]\n\t"
        "v_min_i32 %[mp], %[d0], %[mp]\n\t"
        "v_mul_f32 %[x0], %[m0], %[x0]\n\t"
        "s_nop 1\n\t"
        TFMPC_FWD(0, 1) TFMPC_FWD(0, 2) TFMPC_FWD(0, 3) TFMPC_FWD(0, 4) TFMPC_FWD(0, 5) TFMPC_FWD(0, 6) TFMPC_FWD(0, 7)
        TFMPC_PIVOT(1) TFMPC_VAL(0) "s_nop 0\n\t"
        TFMPC_FWD(1, 2) TFMPC_FWD(1, 3) TFMPC_FWD(1, 4) TFMPC_FWD(1, 5) TFMPC_FWD(1, 6) TFMPC_FWD(1, 7)
        TFMPC_PIVOT(2) TFMPC_VAL(1) "s_nop 0\n\t"
        TFMPC_FWD(2, 3) TFMPC_FWD(2, 4) TFMPC_FWD(2, 5) TFMPC_FWD(2, 6) TFMPC_FWD(2, 7)
        TFMPC_PIVOT(3) TFMPC_VAL(2) "s_nop 0\n\t"
        TFMPC_FWD(3, 4) TFMPC_FWD(3, 5) TFMPC_FWD(3, 6) TFMPC_FWD(3, 7)
        TFMPC_PIVOT(4) TFMPC_VAL(3) "s_nop 0\n\t"
        TFMPC_FWD(4, 5) TFMPC_FWD(4, 6) TFMPC_FWD(4, 7)
        TFMPC_PIVOT(5) TFMPC_VAL(4) "s_nop 0\n\t"
        TFMPC_FWD(5, 6) TFMPC_FWD(5, 7)
        TFMPC_VAL(5)
        TFMPC_PIVOT(6) "s_nop 1\n\t"
        TFMPC_FWD(6, 7)
        TFMPC_VAL(6) "s_nop 0\n\t"
        TFMPC_PIVOT(7) "s_nop 1\n\t"
        TFMPC_VAL(7)
        TFMPC_COPY(m0, 5) TFMPC_COPY(m1, 4)
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
        : [x0] "=&v"(X[0]), [x1] "=&v"(X[1]), [x2] "=&v"(X[2]), [x3] "=&v"(X[3]), [x4] "=&v"(X[4]), [x5] "=&v"(X[5]), [x6] "=&v"(X[6]),
          [x7] "=&v"(X[7]), [m0] "+v"(M[0]), [m1] "+v"(M[1]), [m2] "+v"(M[2]), [m3] "+v"(M[3]), [m4] "+v"(M[4]), [m5] "+v"(M[5]),
          [m6] "+v"(M[6]), [m7] "+v"(M[7]), [mp] "+v"(min_pivot_bits), [acc] "+v"(acc)
        : [d0] "v"(d0));
}
#undef TFMPC_VAL
#undef TFMPC_COPY
#undef TFMPC_BWD
#undef TFMPC_FWD
#undef TFMPC_PIVOT
#undef TFMPC_BC

// ldlt8_solve_neg (wave_ldlt8.h: one system per wave, multipliers as scalars) as its two halves, for the one-wave blocks of the sweep:
// the statements of that routine, unchanged and in its order, with the value chain of the caller -- which reads x^ and m^ -- between them.
// A COPY: wave_ldlt8.h stays as it is for the kernels that share it, so a change to ldlt8_solve_neg there has to be made here as well.  Its
// A/B switch TFMPC_LDLT_SCALAR_FMA is not carried over: it no longer reaches the one-wave blocks of lqr_mfma16x8.hip.
//   M2   in: the lane's column; out: m^ (row p is not touched from pivot p on)
//   N2   out: x^_p = m^_p * rcp(-d_p)
//   nl   out: the multipliers -L[s][p] (s > p), wave-uniform
__device__ __forceinline__ void ldlt8_eliminate_neg(f32x2 (&M2)[4], f32x2 (&N2)[4], float (&nl)[8][8], int &min_pivot_bits)
{
    constexpr int kQuu = 16;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int pp = p >> 1, ps = p & 1;
        const float Mp = M2[pp][ps];
        const int pvb = __builtin_amdgcn_readlane(__builtin_bit_cast(int, Mp), kQuu + p);
        asm("s_min_i32 %0, %0, %1" : "+s"(min_pivot_bits) : "s"(pvb) : "scc");
        const float ninv = __builtin_amdgcn_rcpf(-__builtin_bit_cast(float, pvb));
        const float Mn = Mp * ninv;                      // -row_p / d_p
        N2[pp][ps] = Mn;
#pragma unroll
        for (int s = p + 1; s < 8; ++s)
            nl[s][p] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, Mn), kQuu + s));
        if (ps == 0) M2[pp][1] = fmaf(nl[p + 1][p], Mp, M2[pp][1]);
        const f32x2 Mpp = {Mp, Mp};
#pragma unroll
        for (int k = pp + 1; k < 4; ++k) M2[k] = __builtin_elementwise_fma(f32x2{nl[2 * k][p], nl[2 * k + 1][p]}, Mpp, M2[k]);
    }
}

// X = K~ from x^ (N2, consumed) and the multipliers of the elimination
__device__ __forceinline__ void ldlt8_backsub_neg(f32x2 (&N2)[4], const float (&nl)[8][8], float (&X)[8])
{
#pragma unroll
    for (int s = 7; s >= 1; --s) {
        const float Ns = N2[s >> 1][s & 1];
        const f32x2 Nss = {Ns, Ns};
        if (s & 1) N2[s >> 1][0] = fmaf(nl[s][s - 1], Ns, N2[s >> 1][0]);
#pragma unroll
        for (int k = 0; k < (s >> 1); ++k) N2[k] = __builtin_elementwise_fma(f32x2{nl[s][2 * k], nl[s][2 * k + 1]}, Nss, N2[k]);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) X[r] = N2[r >> 1][r & 1];
}

}  // namespace tfmpc
