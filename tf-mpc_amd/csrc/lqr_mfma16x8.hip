// lqr_mfma16x8.hip -- LQR backward + forward for the BASELINE.json headline shape
// (state_dim n = 16, action_dim m = 8, any horizon) on gfx950 matrix cores; smaller shapes
// (n <= 16, m <= 8) run through the same kernel zero-padded to 16 x 8 (EXACT = false).
//
// Replaces tfmpc/solvers/lqr.py:59-166 of the reference for that shape.  One
// wavefront owns one problem instance for the whole solve.
//
// Backward sweep (lqr.py:73-127), per timestep, all in registers:
//   F~ = [F_x | F_u f 0] (16 x 32) and the tiles of C~ = [[C, c],[.,0]] are loaded once in
//   matrix-core operand layout and stay resident for all T steps.
//   1. W = V F~ (two 16 x 16 tiles; column 24 of W is V f; += v).
//   2. THREE 16 x 16 tiles of Q~ = C~ + F~^T W:  Q_xx = F_x^T W_0;  [Q_uu | q_u] = F~_1^T W_1;
//      and W_1^T F_x, whose rows 0..7 are Q_ux and whose row 8 is q_x^T (V is kept exactly
//      symmetric, step 4, so the F~_1^T W_0 tile is redundant).
//      The accumulator layout of a 16x16 MFMA (lane (j, q) holds rows 4q..4q+3 of column j) IS the
//      operand layout of the next product when the contraction index is enumerated k = 4q + r:
//      W feeds step 2 and V feeds step 1 with no data movement, and one register set of F~ is
//      the B operand of step 1 and the A operand (F~^T) of step 2.
//      Default (BF3): each of these five products is evaluated as "bf16x3" on the bf16 matrix
//      cores -- every fp32 operand split into three bf16 parts (24 mantissa bits), six partial
//      products carried by three v_mfma_f32_16x16x32_bf16 with fp32 accumulation
//      (mfma_bf16x3.h): 15 MFMAs per step.  TFMPC_LQR_MFMA=f32 (tfmpc_set_option) keeps them on
//      v_mfma_f32_16x16x4_f32: 20 MFMAs per step, exact fp32 FMA chains.
//   3. [Q_ux | Q_uu | q_u] (8 x 25) crosses LDS once into "one column per lane, eight rows in
//      registers" and is solved by an LDL^T elimination WITHOUT pivoting that reads only the
//      upper triangle of Q_uu (wave_ldlt8.h; one v_readlane per multiplier serves the forward and
//      the backward sweep) -> K~ = -Q_uu^-1 [Q_ux | q_u].  The reference takes a general
//      inverse (lqr.py:84-87); for a symmetric C with C_uu > 0 (the precondition stated in
//      include/tfmpc_hip.h) Q_uu is SPD and the two agree to rounding.  A non-positive pivot is
//      reported in status[b] (TFMPC_ST_NOT_PD / _SINGULAR).  Launches without value outputs run blocks of TWO waves and one of
//      them eliminates the systems of both instances at once (PAIR below, wave_ldlt8_pair.h): same bits, half the elimination.
//   4. V' = Q_xx + Q_xu K: 2 x v_mfma_f32_16x16x4_f32 (the Schur-complement form of the four-term update
//      lqr.py:97-105, equal to it in exact arithmetic).  v' = q_x + Q_xu k is 128 multiply-adds and gets no matrix tile
//      (a 16 x 16 tile of which one column is used cost two more MFMAs, 64 cycles of the matrix pipe per step): the lanes
//      of the elimination that hold column j of Q_ux finish it from the FORWARD elimination -- with m^_a the reduced row a and
//      x^_a = -m^_a / d_a, v'[j] = q_x[j] + (sum_a x^_a[q_u column] m^_a[j]), which is q_x + Q_xu k written with the factors of Q_uu --
//      as ONE chain of eight FMAs from 0, a = 0..7, and one addition, the same in the paired and in the one-wave blocks, and store it over q_x.  Then
//      V' <- (V' + V'^T) / 2 through an LDS transpose: steps 2 and 3 use the symmetry of V, so its
//      rounding-level antisymmetric part must not survive a step (it would grow like |F_u K|^2
//      per step; the reference does not symmetrise, quirk Q6 of SURVEY.md).
//   K_t, k_t stream to HBM (row-major, the public K/k layout) for the rollout.
// Forward rollout (lqr.py:141-155): wave-wide fp32 FMA mat-vecs with F rows resident in
//   registers, z_t = [x_t; u_t] staged in LDS, K_t prefetched one step ahead, DPP reductions;
//   the stage costs are priced afterwards as C Z on the matrix cores, sixteen steps per tile -- the final cost rides in the last
//   chunk's tiles as one more row with a zeroed action part -- and states / actions leave in bulk coalesced stores.
//
// The f32 MFMA is an exact fp32 FMA chain (MI355X_MICROARCH.md) and bf16x3 drops only terms below
// 2^-24 relative, so numerics are those of fp32 VALU code with a different summation order.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "lqr_kernels.h"
#include "options.h"
#include "mfma_bf16x3.h"
#include "wave_ldlt8.h"
#include "wave_ldlt8_pair.h"
#include "wave_ops.h"

namespace tfmpc {

namespace {

constexpr int N = 16, M = 8, D = 24;
using f32x4 = bf3::f32x4;

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float readlane(float v, int lane)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

using namespace bf3;      // bf16x3 product helpers (mfma_bf16x3.h)

// per-wave LDS slice (floats).  The sweep and the rollout never use it at the same time, so they OVERLAY each other from float 0 and the slice
// is the larger of the two (5 536 B: twelve two-wave blocks fit a CU's 160 KB, where the two laid end to end, 7 584 B, let in ten).
// The __syncthreads() between sweep and rollout orders the two uses: every LDS access of the sweep -- the exchange of the smallest pivots
// included, which is the last time a wave of a paired block touches its PARTNER's slice -- has completed in both waves before either
// writes a rollout row.  Backward-only and forward-only launches use one of the two layouts alone.
//   sweep
// Column stride of the two column-major arrays, in floats (a multiple of 4: 16-byte accesses).  Eight rows are used.  At a stride of 8 (32 B)
// the columns i and i + 4 start on the same one of the 32 banks that dword reads and all stores are spread over, and i and i + 8 on the same
// of the 64 banks of the 8- and 16-byte reads: every access of the step but the transpose's stores was a two- or four-way bank conflict,
// 58 of the 102 LDS-array cycles of an instance's step.  At 12 the 16-byte stores of the staging and both accesses of the paired solve
// are conflict-free and the dword reads of the value update two-way: 56 cycles (tools/probes/lds_banks.py, profiles/r14_mfma16x8_budget.md).
// -DTFMPC_LQR_COLS=8 rebuilds the earlier layout, float for float (A/B builds).
#ifndef TFMPC_LQR_COLS
#define TFMPC_LQR_COLS 12
#endif
constexpr int kCols = TFMPC_LQR_COLS;
// Gains of a step that ran the value update go to HBM from that update's registers (see the gain stores); -DTFMPC_LQR_GAIN_REGS=0 re-reads K~ (A/B builds)
#ifndef TFMPC_LQR_GAIN_REGS
#define TFMPC_LQR_GAIN_REGS 1
#endif
constexpr bool kGainRegs = TFMPC_LQR_GAIN_REGS != 0;
static_assert(kCols % 4 == 0 && kCols >= 8,"columns are 16-byte aligned and hold eight rows; the 32 floats of q_x and the parking row fit columns 28..31");
constexpr int kMs = 0;                    // [32 cols][kCols]  elimination input, column-major
constexpr int kKs = kMs + 32 * kCols;     // [32 cols][kCols]  K~ = -Q_uu^-1 [Q_ux | . | q_u], column-major
constexpr int kVt = kKs + 32 * kCols;     // V' transpose staging [16 cols][kVtLd]
constexpr int kVtLd = 20;
constexpr int kSweepFloats = kVt + 16 * kVtLd;
//   rollout
constexpr int kZs = 0;          // rollout chunk: rows z_t = [x_t(16); u_t(8)], stride kZld
constexpr int kZld = 26;        // even (8-byte aligned rows), 26 n mod 32 distinct for n < 16
#ifndef TFMPC_LQR_TC
#define TFMPC_LQR_TC 52
#endif
constexpr int kTC = TFMPC_LQR_TC;         // timesteps per rollout chunk (T = 50 fits one chunk of 52)
constexpr int kRolloutFloats = kZs + (kTC + 1) * kZld + 6;
constexpr int kLdsFloats = kSweepFloats > kRolloutFloats ? kSweepFloats : kRolloutFloats;
static_assert(kSweepFloats <= kRolloutFloats, "the sweep's layout fits under the rollout's: a wider column stride must not grow the slice (five waves per SIMD)");
static_assert(kLdsFloats % 4 == 0, "slices are 16-byte aligned (pair_src, the 16-byte accesses of the sweep)");
#ifndef TFMPC_LQR_RING
#define TFMPC_LQR_RING 4
#endif
constexpr int kRing = TFMPC_LQR_RING;     // rollout: gains in flight, in steps (the chunk length is a multiple of it: slots keep their phase across chunks)
static_assert(kTC % kRing == 0, "a chunk must hold whole turns of the gain ring");

// DPP lane exchanges inside a row of 16 lanes (no LDS traffic, folded into the VALU op)
template <int CTRL>
__device__ __forceinline__ float dpp(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
constexpr int kDppXor1 = 0xB1;        // quad_perm [1,0,3,2]
constexpr int kDppXor2 = 0x4E;        // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141; // lane i <-> 7 - i inside each 8-lane half row

// Addresses of the time loops (round 8).  A wave-uniform pointer pinned in an SGPR pair and opaque to the compiler: the 32-bit per-lane byte
// offset added to it afterwards stays the VGPR offset of `global_load/store v_off, v_data, s[base:base+1] offset:imm`, and the step advances the
// base on the scalar unit.  Left alone the compiler folds the lane's part into a 64-bit per-lane address ahead of the loop and moves THAT with a
// v_lshl_add_u64 per access and step.
// (The pin hides where the pointer came from, so it is typed as global memory by hand: a generic pointer would be accessed with flat_*.)
#define TFMPC_GLOBAL __attribute__((address_space(1)))
#define TFMPC_LDS __attribute__((address_space(3)))      // (likewise for a volatile LDS access: without it, it goes out as flat_*)
using gbytes = TFMPC_GLOBAL char *;
__device__ __forceinline__ gbytes uniform_base(const float *p)
{
    gbytes g = (gbytes)p;
    asm("" : "+s"(g));
    return g;
}
// The lane's offset is pinned where it is used: widened to 64 bits ahead of the loop it would no longer be recognised as the 32-bit VGPR offset.
// Pinned IN PLACE (the variable itself passes through the empty asm), so that no copy of it is made per use.
__device__ __forceinline__ unsigned here(unsigned &off)
{
    asm volatile("" : "+v"(off));
    return off;
}
template <class V>
__device__ __forceinline__ V gload(gbytes base, unsigned &off) { return *reinterpret_cast<const TFMPC_GLOBAL V *>(base + here(off)); }
template <class V>
__device__ __forceinline__ void gstore(gbytes base, unsigned &off, V v) { *reinterpret_cast<TFMPC_GLOBAL V *>(base + here(off)) = v; }
// A loop-invariant LDS index pinned in a VGPR: its constant part (beyond the offset field of ds_read2 / ds_write2) is added once, not per step.
__device__ __forceinline__ int pinned(int v)
{
    asm("" : "+v"(v));
    return v;
}
// 16-byte row segments of the chunk epilogue: the LDS rows are 8-byte aligned (kZld even), the destination is whatever the caller's pointer is
typedef float f32x4_lds __attribute__((ext_vector_type(4), aligned(8)));
typedef float f32x4_any __attribute__((ext_vector_type(4), aligned(4)));

// EXACT: n == 16 and m == 8 (no guards, vector gain stores).  Otherwise the instance is
// embedded in the 16 x 8 tile grid: states n..15 and actions m..7 are zero rows/columns of
// F~ and C~, with a unit diagonal on the padded part of C_uu so the elimination stays regular
// (the padded gains come out exactly 0).
// OUT16: the 16-bit copies of the policy / value outputs (LqrArgs::K16 ...) are compiled into separate instantiations, so
// that the default kernels carry none of their code
// Register budget (round 4).  Left to itself the compiler takes 105 - 109 VGPRs for the solve kernels: FOUR waves per SIMD (512 / 112).  Sized
// for FIVE (<= 96) the kernels without value-function outputs need 74 - 89 registers and spill nothing -- the LDS slice (7.6 KB then, 5 536 B since the rollout
// overlays the sweep: 29 waves of a CU) is not what limits them -- and the headline launch gains 2 - 4 % on every box tried (tools/probes/r4_headline_eu.sh, alternating: 1.787 -> 1.744 ms, 1.86 ->
// 1.83 ms).  The VALUE instantiations would spill 2 - 19 registers at that budget and keep four.  -DTFMPC_LQR_EU=n forces a budget (A/B builds).
// Round 5: the budget is a template parameter (EU = resident waves per SIMD the register allocation is sized for) and TFMPC_LQR_WAVES=4|5|6
// picks the instantiation at run time, because round 4's verdict suspected the shard sizes of a strong-scaling run to prefer four: 8 192
// instances (the 8-GPU shard of the headline batch) are 8 waves per SIMD = 5 + 3 at five resident, 4 + 4 at four.  Measured on every shard
// size from 1 024 to 65 536 instances (tools/probes/r5_headline_shard_sweep.py, profiles/r05_headline_shard_sweep.json): FIVE wins at each
// of them (8 192: 0.238 against 0.258 ms; the kernel's time is 27.2 us per wave of a SIMD + ~20 us, the rounds overlap because waves do not
// finish together), so five stayed the rule for every launch; six (round 10) is for the paired kernels,
// whose waves wait for each other.  Same instruction stream per wave up to register allocation: bit-identical.
#ifdef TFMPC_LQR_EU
#define TFMPC_LQR_WAVES(EU_) TFMPC_LQR_EU
#else
#define TFMPC_LQR_WAVES(EU_) (EU_)
#endif
#define TFMPC_LQR_OCCUPANCY __attribute__((amdgpu_waves_per_eu(TFMPC_LQR_WAVES(EU), TFMPC_LQR_WAVES(EU))))
// PAIR (round 9): blocks of TWO waves, instance = 2 blockIdx.x + wave, each wave with its own LDS slice.  Everything is still wave-per-
// instance EXCEPT the 8 x 8 elimination: per sweep step ONE wave (the solver, alternating with the step's parity so that the two SIMDs
// share the work) eliminates the systems of both instances at once (wave_ldlt8_pair.h: system A in lanes 0..31, B in lanes 32..63, DPP row
// broadcasts for pivots and multipliers) between two block barriers.  The elimination's instruction count does not depend on how many
// columns ride along, so it is paid once per pair.  EVERY path executes the same number of block barriers in both waves: the second wave
// of an odd last block runs on a clamped instance index with every global store suppressed (`live`), it never exits early.
// Launches without value outputs only: the VALUE / 16-bit instantiations read q_u and k by v_readlane 24 and keep the one-wave block.
// Barrier that orders LDS traffic of the block only (what lds_sync() is to one wave): s_waitcnt lgkmcnt(0) + s_barrier, no vmcnt(0).
__device__ __forceinline__ void block_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
template <bool BACKWARD, bool FORWARD, bool VALUE, bool EXACT, bool BF3, bool OUT16 = false, int EU = 4, bool PAIR = false>
__global__ __launch_bounds__(PAIR ? 2 * kWave : kWave) TFMPC_LQR_OCCUPANCY void lqr_mfma16x8_kernel(LqrArgs a)
{
    static_assert(!PAIR || (BACKWARD && !VALUE && !OUT16), "the paired elimination serves the sweeps without value outputs");
    __shared__ __attribute__((aligned(16))) float lds_all[(PAIR ? 2 : 1) * kLdsFloats];
    const int wave = PAIR ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
    float *const lds = lds_all + wave * kLdsFloats;          // this wave's slice
    const int b_own = PAIR ? 2 * (int)blockIdx.x + wave : (int)blockIdx.x;
    const bool live = !PAIR || b_own < a.B;                  // false: the idle second wave of an odd last block (stores nothing)
    const int b = live ? b_own : a.B - 1;
    const int lane = PAIR ? (int)(threadIdx.x & (kWave - 1)) : (int)threadIdx.x;
    const int i = lane & 15, q = lane >> 4;
    const int T = a.T;
    const int n = EXACT ? N : a.n, m = EXACT ? M : a.m, d = n + m;
    // padded-index accessors: x index xi in [0,16), u index ui in [0,8)
    auto Fxx = [&](const float *Fg, int row, int xi) { return (row < n && xi < n) ? Fg[row * d + xi] : 0.0f; };
    auto Fxu = [&](const float *Fg, int row, int ui) { return (row < n && ui < m) ? Fg[row * d + n + ui] : 0.0f; };
    // z index zi in [0,24): 0..15 -> x, 16..23 -> u; returns the real row/col of C, c or -1
    auto zmap = [&](int zi) { return zi < N ? (zi < n ? zi : -1) : (zi - N < m ? n + zi - N : -1); };
    auto Czz = [&](const float *Cg, int zr, int zc) {
        const int r = zmap(zr), c_ = zmap(zc);
        return (r >= 0 && c_ >= 0) ? Cg[r * d + c_] : 0.0f;
    };
    auto cz = [&](const float *cg, int zr) { const int r = zmap(zr); return r >= 0 ? cg[r] : 0.0f; };
    const float *Fg = a.F + (size_t)b * a.sF;
    const float *fg = a.f + (size_t)b * a.sf;
    const float *Cg = a.C + (size_t)b * a.sC;
    const float *cg = a.c + (size_t)b * a.sc;
    float *Kg = a.K + (size_t)b * a.sK;
    float *kg = a.k + (size_t)b * a.sk;
    int status = 0;

    if (BACKWARD) {
        // ---- resident operands ------------------------------------------------------
        float Fb0[4], Fb1[4];            // F~_c[4q+r][i]
        f32x4 Cd00, Cd11;                // C~[16a+4q+r][16c+i]
        f32x4 Cd01t;                     // rows 0..7: C_ux, row 8: c_x  (= (C~ tile (0,1))^T)
        f32x4 vterm;                     // c_x in lanes i == 8 (terminal v)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 4 * q + r;         // state row of F~ / row of the x-part of C~
            const int ku = N + k;            // z index of the u-part rows (16..31; 16..23 exist)
            if (EXACT) {
                Fb0[r] = Fg[k * D + i];
                Fb1[r] = (i < M) ? Fg[k * D + N + i] : ((i == M) ? fg[k] : 0.0f);
                Cd00[r] = Cg[k * D + i];
                Cd01t[r] = (k < M) ? Cg[(N + k) * D + i] : ((k == M) ? cg[i] : 0.0f);     // C~[16+k][i] | c_x
                vterm[r] = (i == M) ? cg[k] : 0.0f;
                Cd11[r] = (ku < D) ? ((i < M) ? Cg[ku * D + N + i] : ((i == M) ? cg[ku] : 0.0f)) : 0.0f;
            } else {
                Fb0[r] = Fxx(Fg, k, i);
                Fb1[r] = (i < M) ? Fxu(Fg, k, i) : ((i == M && k < n) ? fg[k] : 0.0f);
                Cd00[r] = Czz(Cg, k, i);
                Cd01t[r] = (k < M) ? Czz(Cg, N + k, i) : ((k == M) ? cz(cg, i) : 0.0f);
                vterm[r] = (i == M) ? cz(cg, k) : 0.0f;
                float c11 = 0.0f;
                if (ku < D) {
                    if (i < M) c11 = (k >= m && i == k) ? 1.0f : Czz(Cg, ku, N + i);   // unit diagonal on padded actions
                    else if (i == M) c11 = cz(cg, ku);
                }
                Cd11[r] = c11;
            }
        }
        ConstFrag Fc0{}, Fc1{};                  // bf16x3 fragments of F~ (BF3 only)
        if (BF3) {
            Fc0 = const_frag(f32x4{Fb0[0], Fb0[1], Fb0[2], Fb0[3]});
            Fc1 = const_frag(f32x4{Fb1[0], Fb1[1], Fb1[2], Fb1[3]});
        }
        // terminal value function V = C_xx, v = c_x (lqr.py:67-68): v lives in lanes i == 8
        f32x4 Vd = Cd00, vd = vterm;
        float cst = 0.0f;
        int min_pivot_bits = 0x3f800000;     // smallest pivot seen, as float bits (int order == float order for >= 0)
        int min_pivot_rows = 0x3f800000;     // PAIR: per lane, over the steps THIS wave eliminated (lanes 0..31: instance of wave 0, 32..63: of wave 1)
        // PAIR: the solver's column of either slice.  Row of 16 lanes r = 0, 1 of system s = lane >> 5: lane 0 holds q_u, lanes 1..7 the
        // columns 1..7 of Q_uu, lanes 8..15 the columns 8r .. 8r+7 of Q_ux.  K~ goes back to the same column of the slice (column 24 from both rows,
        // with equal values), and the lanes of Q_ux column j turn q_x[j] into v'[j] in place (pair_qx; step 4).
        const int pj = lane & 15, prow = (lane >> 4) & 1;
        const int pcol = pj >= 8 ? pj - 8 + 8 * prow : (pj == 0 ? N + M : N + pj);
        const int pair_src = PAIR ? 4 * pinned(((lane >> 5) * kLdsFloats + kMs + pcol * kCols) / 4) : 0;       // (a multiple of 4 floats by construction: 16-byte LDS accesses)
        const int pair_d0 = (lane >> 5) * kLdsFloats + kMs + N * kCols;      // Q_uu[0][0] of the lane's system
        constexpr int kZero = kMs + 25 * kCols;  // columns 25..31 of the elimination input are never written by step 3
        // ... and are the only part of the slice that is read before it is written: column 25 as the zero operand (t01_src below), all of
        // them by the elimination's lanes 25..31 (whose results nobody reads; the paired elimination reads columns 0..24 only).  So the
        // whole tail of the array, from column 25 to its end at any stride, is zeroed here once.  q_x, then v', overwrites the 16 floats
        // from column 28 on every step, and in a paired launch the solver's Q_uu lanes park their (meaningless) chain results in the 16
        // floats behind those, which nothing reads there (at stride 8 these are the columns 28, 29 and 30, 31; at a wider stride the 32
        // floats end inside column 30: they are addressed as one run of floats, not as columns, the tail being contiguous at any
        // stride); every step writes the rows 0..7 of the columns 0..24 of the input and of every column of K~ that is read (PAIR: 0..15
        // and 24, else all) before it reads them, and the transpose staging likewise; rows 8.. of a column are never read.  Column 25
        // stays zero.
        for (int z = kZero + lane; z < kKs; z += kWave) lds[z] = 0.0f;
        constexpr int kQx = kMs + 28 * kCols;    // q_x staging, 16 floats (16-byte aligned: t01_src); v' takes its place behind the elimination
        constexpr int kPark = kQx + 16;          // parking, 16 floats: with q_x one run of 32 floats, so that pair_qx covers the 32 banks once
        static_assert(kPark + 16 <= kKs, "q_x and the parking floats lie inside the tail of the elimination input");
        const int pair_qx = (lane >> 5) * kLdsFloats + (pj >= 8 ? kQx + pj - 8 + 8 * prow : kPark + pj + 8 * prow);
        const int t01_src = (i == M) ? kQx + 4 * q : kZero;
        // loop-invariant addresses of the step (pinned: see above)
        const int g0_src = pinned(kKs + i * kCols + q);              // K[4s+q][i]
        const int vt_dst = pinned(kVt + 4 * q * kVtLd + i);          // V' transpose staging, element [row 4q][column i]
        unsigned offK = 8u * lane, offk = 4u * lane;                 // byte offsets of this lane's gains inside a step (EXACT)
        __syncthreads();

        // One sweep step.  LAST (a std::bool_constant) marks the step t == 0 of a launch without value outputs, peeled below: nothing reads
        // its V', v', so it ends at its gains.
        auto sweep_step = [&](const int t, auto LAST) __attribute__((always_inline)) {
            // 1. W = V F~ (+ v on column 24)                                  lqr.py:74,77-78
            //    v enters W_1 as the accumulator of its product (vd is zero outside lanes i == 8, see step 4): no add
            f32x4 W0 = {0.f, 0.f, 0.f, 0.f}, W1 = vd;
            if (BF3) {
                const VarFrag Vf = var_frag_block(Vd);
                W0 = mm_var_const(Vf, Fc0, W0);
                W1 = mm_var_const(Vf, Fc1, W1);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    W0 = mfma(Vd[r], Fb0[r], W0);
                    W1 = mfma(Vd[r], Fb1[r], W1);
                }
            }
            float fw = 0.0f, fv = 0.0f;
            if (VALUE) {     // f^T (V f + v) and f^T v for the const recursion (lqr.py:120); W_1 itself is what every instantiation computes
                float pw = 0.0f, pv = 0.0f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pw = fmaf(Fb1[r], W1[r], pw);
                    pv = fmaf(Fb1[r], vd[r], pv);
                }
                fw = wave_sum(i == M ? pw : 0.0f);
                fv = wave_sum(i == M ? pv : 0.0f);
            }
            // 2. Q~ = C~ + F~^T W                                              lqr.py:75-78
            // Three tiles: Q_xx = F_x^T W_0; [Q_uu | q_u] = F~_1^T W_1; and W_1^T F_x, whose rows
            // 0..7 are Q_ux (= F_u^T V F_x: V is kept exactly symmetric, step 4, so this equals the
            // F~_1^T W_0 tile that is no longer computed) and whose row 8 is q_x^T = (V f + v)^T F_x.
            f32x4 T00 = Cd00, T01t = Cd01t, T11 = Cd11;
            if (BF3) {
                const VarFrag W0f = var_frag_block(W0), W1f = var_frag_block(W1);
                T00 = mm_const_var(Fc0, W0f, T00);
                T01t = mm_var_const(W1f, Fc0, T01t);
                T11 = mm_const_var(Fc1, W1f, T11);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    T00 = mfma(Fb0[r], W0[r], T00);
                    T01t = mfma(W1[r], Fb0[r], T01t);
                    T11 = mfma(Fb1[r], W1[r], T11);
                }
            }
            // 3. [Q_ux | Q_uu | q_u] -> column-per-lane layout through LDS; Q_xu and q_x staged
            if (q < 2) {
                *reinterpret_cast<f32x4 *>(&lds[kMs + i * kCols + 4 * q]) = T01t;                // Q_ux[4q+r][i]
                if (i <= M) *reinterpret_cast<f32x4 *>(&lds[kMs + (N + i) * kCols + 4 * q]) = T11;
            } else if (q == 2) {
                lds[kQx + i] = T01t[0];                                                          // q_x[i]
            }
            float quk = 0.0f;
            if constexpr (PAIR) {
                block_lds_sync();            // both slices staged
                if (wave == (t & 1)) {            // the solver of this step
                    f32x2 P2[4];
                    const f32x4 lo = *reinterpret_cast<const f32x4 *>(&lds_all[pair_src]);
                    const f32x4 hi = *reinterpret_cast<const f32x4 *>(&lds_all[pair_src + 4]);
                    const float d0 = lds_all[pair_d0];
                    float vnext = lds_all[pair_qx];                 // q_x[j] in the lanes of Q_ux column j
                    P2[0] = f32x2{lo[0], lo[1]}; P2[1] = f32x2{lo[2], lo[3]};
                    P2[2] = f32x2{hi[0], hi[1]}; P2[3] = f32x2{hi[2], hi[3]};
                    float Pr[8];
                    float corr = 0.0f;                              // sum_a x^_a[q_u] m^_a[j] = (Q_xu k)[j], summed on its own
                    ldlt8_pair_solve_neg(P2, Pr, d0, min_pivot_rows, corr);
                    lds_all[pair_qx] = vnext + corr;                // v'[j] in place of q_x[j]
                    // K~ of both slices: columns 0..15 = K, column 24 = k (the copies of Q_uu's lanes land in columns 16..23, which nobody reads)
                    f32x4 klo, khi;
#pragma unroll
                    for (int r = 0; r < 4; ++r) { klo[r] = Pr[r]; khi[r] = Pr[4 + r]; }
                    *reinterpret_cast<f32x4 *>(&lds_all[pair_src + (kKs - kMs)]) = klo;
                    *reinterpret_cast<f32x4 *>(&lds_all[pair_src + (kKs - kMs) + 4]) = khi;
                }
                block_lds_sync();            // both K~ written
            } else {
                lds_sync();
                // rows (2k, 2k+1) share a register pair so that one v_pk_fma_f32 updates both
                f32x2 M2[4];
                {
                    const int c = lane & 31;
                    const f32x4 lo = *reinterpret_cast<const f32x4 *>(&lds[kMs + c * kCols]);
                    const f32x4 hi = *reinterpret_cast<const f32x4 *>(&lds[kMs + c * kCols + 4]);
                    M2[0] = f32x2{lo[0], lo[1]}; M2[1] = f32x2{lo[2], lo[3]};
                    M2[2] = f32x2{hi[0], hi[1]}; M2[3] = f32x2{hi[2], hi[3]};
                }
                float vnext = lds[kQx + (lane & 15)];        // q_x[c]
                float qu_saved[8];
                if (VALUE) {
#pragma unroll
                    for (int p = 0; p < 8; ++p) qu_saved[p] = readlane(M2[p >> 1][p & 1], 24);
                }
                // K~ = -Q_uu^-1 [Q_ux | . | q_u]   (lqr.py:84-87; LDL^T on the upper triangle), as the two halves of wave_ldlt8.h's solve
                // (wave_ldlt8_pair.h): the elimination leaves the reduced rows m^ in M2 and x^ = -m^ / d in N2
                f32x2 N2[4];
                float nl[8][8];
                ldlt8_eliminate_neg(M2, N2, nl, min_pivot_bits);
                // v'[c] = q_x[c] + (sum_a x^_a[q_u] m^_a[c]) in place of q_x[c]: the chain of the paired solve (wave_ldlt8_pair.h), term for term
                // from 0, and one addition to q_x[c], so that both kinds of block give the same bits
                if constexpr (!decltype(LAST)::value) {
                    float corr = 0.0f;
#pragma unroll
                    for (int p = 0; p < 8; ++p) corr = fmaf(readlane(N2[p >> 1][p & 1], 24), M2[p >> 1][p & 1], corr);
                    vnext += corr;
                    if (lane < N) lds[kQx + lane] = vnext;
                }
                float Mr[8];
                ldlt8_backsub_neg(N2, nl, Mr);
                float kb[8];                     // k = -Q_uu^-1 q_u (column 24), wave-uniform
#pragma unroll
                for (int p = 0; p < 8; ++p) kb[p] = readlane(Mr[p], 24);
                if (VALUE) {
#pragma unroll
                    for (int p = 0; p < 8; ++p) quk = fmaf(kb[p], qu_saved[p], quk);   // k^T q_u
                }
                // K~: columns 0..15 = K, column 24 = k
                if (lane < 32) {
                    f32x4 lo, hi;
#pragma unroll
                    for (int r = 0; r < 4; ++r) { lo[r] = Mr[r]; hi[r] = Mr[4 + r]; }
                    *reinterpret_cast<f32x4 *>(&lds[kKs + lane * kCols]) = lo;
                    *reinterpret_cast<f32x4 *>(&lds[kKs + lane * kCols + 4]) = hi;
                }
                lds_sync();
            }
            // 4. V' = Q_xx + Q_xu K ; v' = q_x + Q_xu k                        lqr.py:97-105
            //    V': contraction over the 8 actions as 2 k-steps, a = 4s + q.
            //    v' was finished by the elimination's lanes (step 3) and stands where q_x stood: lanes i == 8 read their four rows of it,
            //    every other lane reads the always-zero pad column, so the next v is 0 there.
            constexpr bool kFromRegs = kGainRegs && EXACT && !OUT16 && !decltype(LAST)::value;   // (gains to HBM, below)
            float g0r[2] = {0.0f, 0.0f};
            if constexpr (!decltype(LAST)::value) {
                const f32x4 vacc = *reinterpret_cast<const f32x4 *>(&lds[t01_src]);
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const float ax = lds[kMs + i * kCols + 4 * s2 + q];        // Q_xu[i][4s+q] = Q_ux[4s+q][i]
                    const float g0 = lds[g0_src + 4 * s2];                     // K[4s+q][i]
                    T00 = mfma(ax, g0, T00);
                    g0r[s2] = g0;
                }
                // V' <- (V' + V'^T) / 2 (transpose through LDS).  The elimination above reads only the
                // upper triangle of Q_uu; that is consistent only while V carries no antisymmetric part
                // (otherwise the part it ignores, F_u^T a F_u, is missing from the closed-loop product
                // and the rounding-level asymmetry of V grows like |F_u K|^2 per step).
                // Stored element by element as [row 4q+r][column i] (conflict-free: 80 q + i covers the 64 banks once) and read back as ONE
                // 16-byte row segment [row i][4q .. 4q+3] = V'^T, which lands in a register quad that pairs with T00 for the packed adds.
                {
                    const float *vt = &lds[kVt];
#pragma unroll
                    for (int r = 0; r < 4; ++r) lds[vt_dst + r * kVtLd] = T00[r];
                    lds_sync();
                    const f32x4 Tt = *reinterpret_cast<const f32x4 *>(&vt[i * kVtLd + 4 * q]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) Vd[r] = 0.5f * (T00[r] + Tt[r]);
                }
                vd = vacc;
            }
            // gains to HBM, row-major K[t][a][j], k[t][a] (the public layout)
            // A step that ran the value update holds them already (EXACT, no 16-bit copies): lane (i, q) = 16 q + i read K[q][i] and
            // K[4 + q][i] as the g0 operands of step 4, and row-major those are the floats `lane` and 64 + `lane` of K[t] -- two dword
            // stores of 256 contiguous bytes per wave each, no second read of K~.  Same values, same bits.
            if constexpr (kFromRegs) {
                if (live) {
                    const gbytes Kt = uniform_base(Kg + (size_t)t * (M * N));
                    gstore(Kt, offk, g0r[0]);
                    gstore(Kt + 4 * kWave, offk, g0r[1]);
                    if (lane < M) gstore(uniform_base(kg + (size_t)t * M), offk, lds[kKs + 24 * kCols + lane]);
                }
            } else if (live) {
                const int ka = lane >> 3, jc = lane & 7;
                float2 kv;
                kv.x = lds[kKs + (2 * jc) * kCols + ka];
                kv.y = lds[kKs + (2 * jc + 1) * kCols + ka];
                if (EXACT) {
                    gstore(uniform_base(Kg + (size_t)t * (M * N)), offK, f32x2{kv.x, kv.y});
                    if (lane < M) gstore(uniform_base(kg + (size_t)t * M), offk, lds[kKs + 24 * kCols + lane]);
                } else {
                    if (ka < m && 2 * jc < n) Kg[(size_t)t * m * n + ka * n + 2 * jc] = kv.x;
                    if (ka < m && 2 * jc + 1 < n) Kg[(size_t)t * m * n + ka * n + 2 * jc + 1] = kv.y;
                    if (lane < m) kg[(size_t)t * m + lane] = lds[kKs + 24 * kCols + lane];
                }
                if (OUT16 && a.K16) {                      // 16-bit copy of the policy (the rollout reads the fp32 gains)
                    uint16_t *Ko = a.K16 + ((size_t)b * T + t) * (m * n);
                    if (ka < m && 2 * jc < n) Ko[ka * n + 2 * jc] = lqr_to_bf16(kv.x);
                    if (ka < m && 2 * jc + 1 < n) Ko[ka * n + 2 * jc + 1] = lqr_to_bf16(kv.y);
                }
                if (OUT16 && a.k16 && lane < m) a.k16[((size_t)b * T + t) * m + lane] = lqr_to_bf16(lds[kKs + 24 * kCols + lane]);
            }
            if (VALUE) {
                // const += 1/2 k^T Q_uu k + k^T q_u + 1/2 f^T V f + f^T v with Q_uu k = -q_u
                // (lqr.py:113-121); fw = f^T (V f + v) carries one f^T v already: 1/2 f^T V f + f^T v = 1/2 (fw + f^T v).
                cst += 0.5f * quk + 0.5f * (fw + fv);
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
                if (OUT16 && a.V16) {
                    uint16_t *Vo = a.V16 + ((size_t)b * T + t) * (n * n);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (EXACT || (4 * q + r < n && i < n)) Vo[(4 * q + r) * n + i] = lqr_to_bf16(Vd[r]);
                }
                if (OUT16 && a.v16 && i == M) {
                    uint16_t *vo = a.v16 + ((size_t)b * T + t) * n;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (EXACT || 4 * q + r < n) vo[4 * q + r] = lqr_to_bf16(vd[r]);
                }
                if (OUT16 && a.cst16 && lane == 0) a.cst16[(size_t)b * T + t] = lqr_to_bf16(cst);
            }
            lds_sync();
        };
        constexpr int kPeeled = VALUE ? 0 : 1;       // the VALUE instantiations store V', v' of every step
        for (int t = T - 1; t >= kPeeled; --t) sweep_step(t, std::false_type{});
        if (kPeeled && T > 0) sweep_step(0, std::true_type{});
        if constexpr (PAIR) {
            // each wave holds the pivots of the steps it eliminated, for BOTH instances: exchanged through column 25 of K~ (never read or
            // written by the paired step), own slice [instance of wave 0, instance of wave 1]
            constexpr int kMinPv = kKs + 25 * kCols;
            if ((lane & 31) == 0) lds[kMinPv + (lane >> 5)] = __builtin_bit_cast(float, min_pivot_rows);
            block_lds_sync();
            const int p0 = __builtin_bit_cast(int, lds_all[kMinPv + wave]), p1 = __builtin_bit_cast(int, lds_all[kLdsFloats + kMinPv + wave]);
            min_pivot_bits = __builtin_amdgcn_readfirstlane(p0 < p1 ? p0 : p1);
        }
        if (min_pivot_bits <= 0) status |= (min_pivot_bits == 0) ? TFMPC_ST_SINGULAR : TFMPC_ST_NOT_PD;
        if (VALUE && !(cst == cst)) status |= TFMPC_ST_NAN;
    }

    // The rollout takes its lane maps from a lane index of its own, read anew from v_mbcnt (the lane's number inside its wave: what `lane` is in
    // either block shape) and opaque to the compiler: shared with the sweep's, the maps -- and threadIdx.x itself -- would stay alive across the
    // sweep, and at the budget of six waves the sweep has no register to spare for them.  `lane`, `i` and `q` are re-declared ON PURPOSE inside
    // the rollout's block and shadow the sweep's: everything in that block, code added later included, must bind to these.  The status store
    // at the end of the kernel picks its lane by the same index.  (Register counts: profiles/r11_mfma16x8_budget.md.)
    const int lane_rollout = (BACKWARD && FORWARD) ? pinned((int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u))) : lane;
    if (FORWARD) {
        const int lane = lane_rollout, i = lane & 15, q = lane >> 4;
        // ---- resident operands of the rollout ------------------------------------------
        const int fi = lane >> 2, fc = lane & 3;       // F: row fi, columns 6fc..6fc+5
        const int ka = lane >> 3, jc = lane & 7;       // K: row ka, columns 2jc, 2jc+1
        float Fr[6];
        if (EXACT) {
            const float2 *p = reinterpret_cast<const float2 *>(Fg + fi * D + 6 * fc);
#pragma unroll
            for (int j = 0; j < 3; ++j) { const float2 v = p[j]; Fr[2 * j] = v.x; Fr[2 * j + 1] = v.y; }
        } else {
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int zc = 6 * fc + j;
                Fr[j] = zc < N ? Fxx(Fg, fi, zc) : Fxu(Fg, fi, zc - N);
            }
        }
        const float f_part = (fc == 0 && (EXACT || fi < n)) ? fg[fi] : 0.0f;     // f enters one of the four partial sums
        // cost post-pass operands: A = C (2 row tiles x 6 k-steps, k = 4s + q), c in D layout
        float Ca0[6], Ca1[6];
        f32x4 cq0, cq1;
#pragma unroll
        for (int s2 = 0; s2 < 6; ++s2) {
            if (EXACT) {
                Ca0[s2] = Cg[i * D + 4 * s2 + q];
                Ca1[s2] = (i < M) ? Cg[(N + i) * D + 4 * s2 + q] : 0.0f;
            } else {
                Ca0[s2] = Czz(Cg, i, 4 * s2 + q);
                Ca1[s2] = (i < M) ? Czz(Cg, N + i, 4 * s2 + q) : 0.0f;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            cq0[r] = EXACT ? cg[4 * q + r] : cz(cg, 4 * q + r);
            cq1[r] = (q < 2) ? (EXACT ? cg[N + 4 * q + r] : cz(cg, N + 4 * q + r)) : 0.0f;
        }
        float *xs = a.states + (size_t)b * (T + 1) * n;
        float *us = a.actions + (size_t)b * T * m;
        float *cs = a.costs + (size_t)b * (T + 1);
        float *zs = &lds[kZs];
        __syncthreads();                               // gains written above are visible
        if (lane < N) {
            const float x = (EXACT || lane < n) ? a.x0[(size_t)b * n + lane] : 0.0f;
            zs[lane] = x;
            if (live && (EXACT || lane < n)) xs[lane] = x;
        }
        // gains of step t for this lane: K[ka][2jc], K[ka][2jc+1], k[ka]
        // EXACT: one per-lane byte offset each for K and k, fixed for the whole rollout; the (clamped, wave-uniform) step moves an SGPR base
        unsigned offK = 8u * lane, offk = 4u * ka;
        auto load_gain = [&](int t, float2 &Kv, float &kv) {
            if (EXACT) {
                const f32x2 K2 = gload<f32x2>(uniform_base(Kg + (size_t)t * (M * N)), offK);
                Kv = float2{K2[0], K2[1]};
                kv = gload<float>(uniform_base(kg + (size_t)t * M), offk);
            } else {
                const bool row = ka < m;
                Kv.x = (row && 2 * jc < n) ? Kg[(size_t)t * m * n + ka * n + 2 * jc] : 0.0f;
                Kv.y = (row && 2 * jc + 1 < n) ? Kg[(size_t)t * m * n + ka * n + 2 * jc + 1] : 0.0f;
                kv = row ? kg[(size_t)t * m + ka] : 0.0f;
            }
        };
        // Register ring kRing steps deep, statically indexed through the unrolled inner loop below (round 6): a rotation through copies
        // at the loop's back edge makes the compiler wait for the load it has just issued -- one memory round trip per step.
        float2 KR[kRing];
        float kR[kRing];
#pragma unroll
        for (int d = 0; d < kRing; ++d) {
            KR[d] = float2{0.f, 0.f};
            kR[d] = 0.0f;
            if (T > 0) load_gain(d < T ? d : T - 1, KR[d], kR[d]);
        }
        __syncthreads();

        // costs of rows [0, rows) of the chunk buffer: 1/2 z^T C z + c^T z  (lqr.py:41-47)
        // as C Z on the matrix cores, 16 timesteps per tile.  Every cost is computed from its own row alone (column i of the tile), whatever
        // the other columns hold.  Returns the costs of the LAST tile, row 16 nt + i in the lanes of column i.
        auto chunk_costs = [&](int rows, float *out) {
            float part = 0.0f;
            for (int nt = 0; nt * 16 < rows; ++nt) {
                const int row = (16 * nt + i < rows) ? 16 * nt + i : rows - 1;    // stay inside the chunk
                const float *zrow = zs + row * kZld;
                f32x4 D0 = {0.f, 0.f, 0.f, 0.f}, D1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s2 = 0; s2 < 6; ++s2) {
                    const float bz = zrow[4 * s2 + q];
                    D0 = mfma(Ca0[s2], bz, D0);
                    D1 = mfma(Ca1[s2], bz, D1);
                }
                part = 0.0f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    part = fmaf(zrow[4 * q + r], fmaf(0.5f, D0[r], cq0[r]), part);
                    if (q < 2) part = fmaf(zrow[N + 4 * q + r], fmaf(0.5f, D1[r], cq1[r]), part);
                }
                part += __shfl_xor(part, 16, kWave);
                part += __shfl_xor(part, 32, kWave);
                if (live && q == 0 && 16 * nt + i < rows) {
                    unsigned offc = 4u * lane;        // (q == 0: lane == i)
                    gstore(uniform_base(out + 16 * nt), offc, part);
                }
            }
            return part;
        };

        // One rollout step: row tt of the chunk buffer, step t of the horizon, gains from one slot of the ring.
        auto rollout_step = [&](const int tt, const int t, float2 &KRd, float &kRd, auto REFILL) __attribute__((always_inline)) {
            float *zt = zs + tt * kZld;
            const float2 Kc = KRd;
            const float kc = kRd;
            // u = K x + k                                              lqr.py:143
            const float2 xv = *reinterpret_cast<const float2 *>(&zt[2 * jc]);
            float u = fmaf(Kc.x, xv.x, Kc.y * xv.y);
            u += dpp<kDppXor1>(u);
            u += dpp<kDppXor2>(u);
            u += dpp<kDppHalfMirror>(u);
            u += kc;
            // this slot's next step -- UNCONDITIONAL (clamped: the last turns reload the final step): behind a branch the compiler
            // can no longer count the loads in flight and waits for all of them.  Issued once the slot's gains are consumed, so that it is
            // refilled IN PLACE (issued ahead of them the new gains need registers of their own and are copied into the slot afterwards).
            if constexpr (decltype(REFILL)::value) load_gain(t + kRing < T ? t + kRing : T - 1, KRd, kRd);
            zt[N + ka] = u;                      // all eight lanes of the row hold the same sum
            lds_sync();
            // x' = F z + f                                              lqr.py:36-39
            float xn = f_part;
            const float2 *zp = reinterpret_cast<const float2 *>(&zt[6 * fc]);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float2 z2 = zp[j];
                xn = fmaf(Fr[2 * j], z2.x, xn);
                xn = fmaf(Fr[2 * j + 1], z2.y, xn);
            }
            xn += dpp<kDppXor1>(xn);
            xn += dpp<kDppXor2>(xn);
            zt[kZld + fi] = xn;                  // likewise: the four lanes of row fi agree
            lds_sync();
        };

        // chunk epilogue (EXACT): 16 bytes per lane -- four lanes per state row (64 B), two per action row (32 B); sources fixed per lane
        const int xrow = lane >> 2, urow = lane >> 1;
        const float *xsrc = zs + (1 + xrow) * kZld + 4 * (lane & 3);
        const float *usrc = zs + urow * kZld + N + 4 * (lane & 1);
        unsigned off16 = 16u * lane;
        // rows of the chunk an iteration of the stores still has ahead of it, opaque to the compiler: it would fold the two tests on it into
        // one per-lane bound per iteration and keep those in registers across the chunk
        auto rows_left = [](int v) { asm("" : "+s"(v)); return v; };

        // (T = 0 runs the loop once with no step: its one row is x_0, priced as the final cost)
        for (int t0 = 0; t0 == 0 || t0 < T; t0 += kTC) {
            const bool last = T - t0 <= kTC;
            const int tc = last ? T - t0 : kTC;
            int tb = 0;
            for (; tb + kRing <= tc; tb += kRing) {
#pragma unroll
                for (int d = 0; d < kRing; ++d) rollout_step(tb + d, t0 + tb + d, KR[d], kR[d], std::true_type{});
            }
            // Fewer than kRing steps are left in the LAST chunk only (every other chunk is whole turns of the ring, so slot d still holds step
            // tb + d): they take their gains from their slots and refill nothing.  Kept out of the loop above: an exit from the middle of a turn
            // makes the compiler rotate the ring through copies at the back edge.
#pragma unroll
            for (int d = 0; d < kRing - 1; ++d)
                if (tb + d < tc) rollout_step(tb + d, t0 + tb + d, KR[d], kR[d], std::false_type{});
            // chunk epilogue: stage costs on the matrix cores, bulk coalesced stores.
            // The LAST chunk prices the final cost 1/2 x_T^T C_xx x_T + c_x^T x_T == stage cost with u = 0 (lqr.py:49-57) in the same tiles:
            // row tc of the buffer holds x_T (the last step put it there, or the prologue at T = 0), and its action part -- never written, or a
            // stale action of an earlier chunk -- is zeroed here.  Nothing else reads those eight floats: the action stores below read rows 0..tc-1.
            if (last) {
                if (lane < M) zs[tc * kZld + N + lane] = __builtin_bit_cast(float, pinned(0));     // (a zero made here: one shared with the loop would live across it)
                lds_sync();
            }
            const float tile_costs = chunk_costs(last ? tc + 1 : tc, cs + t0);       // row tc goes to cs[t0 + tc] == cs[T]
            if (last) {
                // the final cost as the lane that stored it holds it: nobody reads cs[T] back
                const float fcost = readlane(tile_costs, tc & 15);
                if (!(fcost == fcost)) status |= TFMPC_ST_NAN;
            }
            if (!live) {
                // the idle wave of an odd last block stores nothing
            } else if (EXACT) {
                // rows 1..tc of the buffer are x_{t0+1..t0+tc}, rows 0..tc-1 hold u_{t0..t0+tc-1}: every iteration is one LDS read and one
                // store at immediate offsets from a fixed source and a chunk-uniform destination, the row guard stores exactly tc rows
                const gbytes xdst = uniform_base(xs + (size_t)(t0 + 1) * N), udst = uniform_base(us + (size_t)t0 * M);
#pragma unroll
                for (int r0 = 0; r0 < kTC; r0 += kWave / 4) {
                    const int left = rows_left(tc - r0);
                    if (left <= 0) break;
                    if (xrow < left)
                        gstore<f32x4_any>(xdst + r0 * (N * 4), off16, *reinterpret_cast<const f32x4_lds *>(xsrc + r0 * kZld));
                }
#pragma unroll
                for (int r0 = 0; r0 < kTC; r0 += kWave / 2) {
                    const int left = rows_left(tc - r0);
                    if (left <= 0) break;
                    if (urow < left)
                        gstore<f32x4_any>(udst + r0 * (M * 4), off16, *reinterpret_cast<const f32x4_lds *>(usrc + r0 * kZld));
                }
            } else {
                for (int idx = lane; idx < tc * n; idx += kWave)
                    xs[(size_t)(t0 + 1) * n + idx] = zs[(1 + idx / n) * kZld + idx % n];
                for (int idx = lane; idx < tc * m; idx += kWave)
                    us[(size_t)t0 * m + idx] = zs[(idx / m) * kZld + N + idx % m];
            }
            if (!last) {
                lds_sync();
                if (lane < N) zs[lane] = zs[kTC * kZld + lane];      // carry x into row 0 of the next chunk
                lds_sync();
            }
        }
    }

    // `status` is wave-uniform here: the pivot bits come out of a v_readfirstlane, `cst` is a wave sum, and the final cost's NaN test reads one
    // lane's value with v_readlane in every lane -- whichever lane stores it stores the same word.
    if (live && a.status && lane_rollout == 0) a.status[b] = status;
}

// TFMPC_LQR_MFMA=f32 keeps the two big products of the sweep on the f32 MFMA; the default
// evaluates them as bf16x3 on the bf16 matrix cores (same fp32-level accuracy, see split3).
bool use_bf16x3()
{
    return !option_is(kOptLqrMfma, "f32");
}

// Register budget of a launch without value outputs: five waves per SIMD (see the note above the kernel); TFMPC_LQR_WAVES=4|5|6 forces
// (A/B timing, the bit-identity tests).  Six is served by the paired kernels only (80 VGPRs; the slice of 5 536 B lets twelve two-wave
// blocks into a CU) and stays an option: it has to beat five by the project's bar in every session taken, and against the shortened
// elimination it no longer does in any (profiles/r10_mfma16x8_budget.md, profiles/r11_mfma16x8_budget.md).
int pick_eu()
{
    const int forced = option_int(kOptLqrWaves, 0);
    return forced == 4 || forced == 6 ? forced : 5;
}

template <bool BW, bool FW, bool VAL, bool O16, int EU>
int launch_eu(const LqrArgs &a, hipStream_t stream)
{
    const bool exact = a.n == N && a.m == M;
    const bool bf3 = BW && use_bf16x3();
    // sweeps without value outputs: blocks of two waves that share the elimination (PAIR, see the kernel)
    constexpr bool P = BW && !VAL && !O16;
    const dim3 grid(P ? (a.B + 1) / 2 : a.B), block(P ? 2 * kWave : kWave);
    if (exact && bf3) hipLaunchKernelGGL((lqr_mfma16x8_kernel<BW, FW, VAL, true, true, O16, EU, P>), grid, block, 0, stream, a);
    else if (exact) hipLaunchKernelGGL((lqr_mfma16x8_kernel<BW, FW, VAL, true, false, O16, EU, P>), grid, block, 0, stream, a);
    else if (bf3) hipLaunchKernelGGL((lqr_mfma16x8_kernel<BW, FW, VAL, false, true, O16, EU, P>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((lqr_mfma16x8_kernel<BW, FW, VAL, false, false, O16, EU, P>), grid, block, 0, stream, a);
    return hipGetLastError() == hipSuccess ? TFMPC_OK : TFMPC_ERR_LAUNCH;
}

template <bool BW, bool FW, bool VAL, bool O16 = false>
int launch(const LqrArgs &a, hipStream_t stream)
{
    // the VALUE instantiations would spill at the budget for five (round 4): they keep four
    if constexpr (!VAL) {
        const int eu = pick_eu();
        // six: the paired kernels only (their waves wait for each other, and a sixth covers the waiters); the others keep five
        if constexpr (BW && !O16) {
            if (eu == 6) return launch_eu<BW, FW, VAL, O16, 6>(a, stream);
        }
        if (eu >= 5) return launch_eu<BW, FW, VAL, O16, 5>(a, stream);
    }
    return launch_eu<BW, FW, VAL, O16, 4>(a, stream);
}

}  // namespace

// Exact headline shape, or any smaller shape that is still worth a 16 x 8 tile grid (below
// n + m = 7 the lane-per-instance kernel of lqr_lane.hip takes over).
bool lqr_mfma_supported(int n, int m) { return n >= 1 && m >= 1 && n <= N && m <= M && n + m > 6; }

int lqr_mfma_launch(const LqrArgs &a, bool backward, bool forward, hipStream_t stream)
{
    if (a.K16 || a.k16 || a.V16 || a.v16 || a.cst16) {       // 16-bit outputs: the value-function code is compiled in
        if (backward && forward) return launch<true, true, true, true>(a, stream);
        if (backward) return launch<true, false, true, true>(a, stream);
    }
    const bool value = a.V || a.v || a.cst;
    if (backward && forward) return value ? launch<true, true, true>(a, stream) : launch<true, true, false>(a, stream);
    if (backward) return value ? launch<true, false, true>(a, stream) : launch<true, false, false>(a, stream);
    return launch<false, true, false>(a, stream);
}

}  // namespace tfmpc
