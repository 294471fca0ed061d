// tvlqr_wave.h -- the ONE body of the wave-per-instance time-varying LQR: LDS layout, backward
// sweep, rollout and launcher, instantiated in fp32 by tvlqr_generic.hip and in double by tvlqr_f64.hip (whole horizons,
// and single segments for the expand phases of the time-parallel solve, DESIGN.md 3.19, and of the periodic steady
// state, 3.25: there the backward sweep alone).
//
// Per step t of the backward sweep the wave copies F_t, f_t, C_t, c_t into its LDS slice and runs the symmetric
// recursion of the fast kernels: W = F_t^T V, Q = C_t + W F_t and V' = Q_xx + Q_xu K on the matrix cores, q = c_t + W f_t
// + F_t^T v, v' = q_x + Q_xu k and const on the vector unit, Q_uu eliminated WITHOUT pivoting (a non-positive pivot <=>
// Q_uu not positive definite: TFMPC_ST_NOT_PD), V' symmetrised.  The rollout copies F_t, f_t, C_t, c_t, K_t, k_t per
// step.  Nothing is prefetched.  The split backward + forward launches and the fused solve run the same device function
// and give the same bits.
//
// A policy P carries what differs between the precisions and nothing else:
//   P::T, P::matmul     the scalar type and the matrix-core product: WaveF32 or WaveF64<MAXD> (wave_ops_f64.h)
//   P::kFold            the LDS layout (TvSmem below)
//   P::valid(x)         the status test: const or the final cost failing it sets TFMPC_ST_NAN
// The status test is an existing difference that is kept: fp32 flags NaN only, double flags NaN or infinity.
#pragma once

#include <hip/hip_runtime.h>

#include "lqr_kernels.h"
#include "tvlqr_kernels.h"
#include "wave_ops_f64.h"

namespace tfmpc {

// The body names s.Q, s.Vn (leading dimension ldv) and s.aug and never asks which layout it has.  Unfolded, every
// buffer is its own.  FOLD (LDS, not registers, sets the resident waves in double): Q lies over C_t (each
// lane replaces the element it read as the product's initial value), V' over Q_xx in the same way, the elimination's
// augmented system takes W's place once Q and q are formed, and there is no prow.
template <class S>
struct TvSmem {
    int ldd, ldn, lda, ldv, width;
    S *F, *f, *C, *c, *V, *v, *W, *Q, *q, *aug, *fac, *prow, *K, *k, *Vn, *vn, *z, *xn;
};

// folded: the one buffer that holds W = F^T V, then aug
__host__ __device__ constexpr size_t tv_fold_w_elems(int n, int m)
{
    const size_t w = (size_t)(n + m) * odd_ld(n), aug = (size_t)m * odd_ld(m + 1 + n);
    return w > aug ? w : aug;
}

template <bool FOLD>
__host__ __device__ constexpr size_t tv_smem_elems(int n, int m)
{
    const int d = n + m;
    const int ldd = odd_ld(d), ldn = odd_ld(n), width = m + 1 + n, lda = odd_ld(width);
    size_t s = 0;
    s += (size_t)n * ldd + n;                                  // F, f
    s += (size_t)d * ldd + d;                                  // C, c
    s += (size_t)n * ldn + n;                                  // V, v
    if (FOLD) s += tv_fold_w_elems(n, m);                      // W, then aug
    else s += (size_t)d * ldn + (size_t)m * lda + width;       // W, aug, prow
    if (!FOLD) s += (size_t)d * ldd + (size_t)n * ldn;         // Q, Vn
    s += (size_t)d + m;                                        // q, fac
    s += (size_t)m * ldn + m;                                  // K, k
    s += (size_t)n;                                            // vn
    s += (size_t)d + n;                                        // z, xn
    return s;
}

template <bool FOLD, class S>
__device__ inline TvSmem<S> tv_carve(S *base, int n, int m)
{
    TvSmem<S> s;
    const int d = n + m;
    s.ldd = odd_ld(d);
    s.ldn = odd_ld(n);
    s.width = m + 1 + n;
    s.lda = odd_ld(s.width);
    S *p = base;
    s.F = p; p += n * s.ldd;
    s.f = p; p += n;
    s.C = p; p += d * s.ldd;
    s.c = p; p += d;
    s.V = p; p += n * s.ldn;
    s.v = p; p += n;
    s.W = p;
    if (FOLD) { s.Q = s.C; s.aug = s.W; p += tv_fold_w_elems(n, m); }
    else { p += d * s.ldn; s.Q = p; p += d * s.ldd; }
    s.q = p; p += d;
    if (!FOLD) { s.aug = p; p += m * s.lda; }
    s.fac = p; p += m;
    s.prow = nullptr;
    if (!FOLD) { s.prow = p; p += s.width; }
    s.K = p; p += m * s.ldn;
    s.k = p; p += m;
    if (FOLD) { s.Vn = s.Q; s.ldv = s.ldd; }
    else { s.Vn = p; s.ldv = s.ldn; p += n * s.ldn; }
    s.vn = p; p += n;
    s.z = p; p += d;
    s.xn = p; p += n;
    return s;
}

// Which part of which instance a wave works on.  TvWhole: instance blockIdx.x, the whole horizon -- every constant below
// folds and the body is the one it was.  TvSegment (the time-parallel solve's expand phase): steps
// t0 .. t0 + len - 1 of instance b, the value function behind the segment and the state at its start read from the
// stitch's workspace; only the LAST segment writes states[T] and the final cost.
struct TvWhole {
    static constexpr bool kSegment = false;
};
template <class S>
struct TvSegment {
    static constexpr bool kSegment = true;
    int b, t0, len;
    bool last;
    const S *Vend, *vend;         // [n][n], [n]: the value function at step t0 + len
    const S *xstart;              // [n]: the state at step t0
    int32_t *status;              // this wave's own status word
};

// MASKED (in double 3.20): held controls (bit i of a.mask[b][t]) are taken out of the step's model after
// the LDS copy.
template <class P, bool BACKWARD, bool FORWARD, bool MASKED, class SEG = TvWhole>
__device__ __forceinline__ void tvlqr_wave_body(const TvLqrArgsT<typename P::T> &a, typename P::T *smem, const SEG &seg = SEG())
{
    using S = typename P::T;
    static_assert(!MASKED || !SEG::kSegment, "the masked sweep runs whole horizons");
    int b;
    if constexpr (SEG::kSegment) b = seg.b;
    else b = blockIdx.x;
    const int lane = lane_id();
    const int n = a.n, m = a.m, d = n + m, Th = a.T;         // Th: the whole horizon, the outputs' layout
    int T = Th;                                               // the steps of this wave
    if constexpr (SEG::kSegment) T = seg.len;
    // step t of this wave in the horizon (written so that the whole-horizon kernels see the very expressions they had)
    auto at = [&](int t) {
        if constexpr (SEG::kSegment) return seg.t0 + t;
        else return t;
    };
    auto last_step = [&]() {
        if constexpr (SEG::kSegment) return Th - 1;
        else return T - 1;
    };
    TvSmem<S> s = tv_carve<P::kFold>(smem, n, m);
    const int ldd = s.ldd, ldn = s.ldn, lda = s.lda, ldv = s.ldv;
    auto load_model = [&](int t) {
        load_matrix(s.F, ldd, tv_at(a.F, a.sF_b, a.sF_t, b, at(t)), n, d);
        load_matrix(s.C, ldd, tv_at(a.C, a.sC_b, a.sC_t, b, at(t)), d, d);
        const S *fg = tv_at(a.f, a.sf_b, a.sf_t, b, at(t)), *cg = tv_at(a.c, a.sc_b, a.sc_t, b, at(t));
        for (int i = lane; i < n; i += kWave) s.f[i] = fg[i];
        for (int i = lane; i < d; i += kWave) s.c[i] = cg[i];
    };
    // the final cost's (C_fin, c_fin, leading dimension): explicit, or C_{T-1}[:n,:n], c_{T-1}[:n]
    const S *Cf = a.Cfin ? a.Cfin + (size_t)b * a.sCfin_b : tv_at(a.C, a.sC_b, a.sC_t, b, last_step());
    const S *cf = a.Cfin ? a.cfin + (size_t)b * a.scfin_b : tv_at(a.c, a.sc_b, a.sc_t, b, last_step());
    const int ldf = a.Cfin ? n : d;
    // where the backward sweep starts: the final cost, or the value function behind the segment
    const S *Vb = Cf, *vb = cf;
    int ldb = ldf;
    if constexpr (SEG::kSegment) { Vb = seg.Vend; vb = seg.vend; ldb = n; }

    int status = 0;
    S *Kg = a.K + (size_t)b * a.sK;
    S *kg = a.k + (size_t)b * a.sk;
    if constexpr (SEG::kSegment) {
        Kg += (size_t)seg.t0 * m * n;
        kg += (size_t)seg.t0 * m;
    }

    if (BACKWARD) {
        wave_for_2d(n, n, [&](int i, int j, int) { s.V[i * ldn + j] = Vb[i * ldb + j]; });
        for (int i = lane; i < n; i += kWave) s.v[i] = vb[i];
        S cst = S(0);
        wsync();

        for (int t = T - 1; t >= 0; --t) {
            load_model(t);
            wsync();
            if (MASKED) {
                const uint32_t w = a.mask[(size_t)b * Th + t];
                auto held = [&](int zi) { return zi >= n && (w >> (zi - n) & 1u); };
                wave_for_2d(n, m, [&](int r, int j, int) { if (w >> j & 1u) s.F[r * ldd + n + j] = S(0); });
                wave_for_2d(d, d, [&](int r, int j, int) { if (held(r) || held(j)) s.C[r * ldd + j] = (r == j) ? S(1) : S(0); });
                for (int r = lane; r < m; r += kWave) if (w >> r & 1u) s.c[n + r] = S(0);
                wsync();
            }
            // W = F_t^T V  [d][n]
            P::matmul(d, n, n,
                        [&](int r, int k) { return s.F[k * ldd + r]; },
                        [&](int k, int j) { return s.V[k * ldn + j]; },
                        [](int, int) { return S(0); },
                        [&](int r, int j, S x) { s.W[r * ldn + j] = x; });
            wsync();
            // Q = C_t + W F_t (over C_t when folded) ; q = c_t + W f_t + F_t^T v
            P::matmul(d, d, n,
                        [&](int r, int k) { return s.W[r * ldn + k]; },
                        [&](int k, int j) { return s.F[k * ldd + j]; },
                        [&](int r, int j) { return s.C[r * ldd + j]; },
                        [&](int r, int j, S x) { s.Q[r * ldd + j] = x; });
            for (int r = lane; r < d; r += kWave) {
                S s1 = S(0), s2 = S(0);
                for (int k = 0; k < n; ++k) {
                    s1 = fma(s.W[r * ldn + k], s.f[k], s1);
                    s2 = fma(s.F[k * ldd + r], s.v[k], s2);
                }
                s.q[r] = s.c[r] + s1 + s2;
            }
            wsync();
            // [Q_uu | q_u | Q_ux] (in W's place when folded) -> Gauss-Jordan without pivoting -> [I | Q_uu^-1 q_u | Q_uu^-1 Q_ux]
            wave_for_2d(m, s.width, [&](int r, int j, int) {
                S x;
                if (j < m) x = s.Q[(n + r) * ldd + n + j];
                else if (j == m) x = s.q[n + r];
                else x = s.Q[(n + r) * ldd + (j - m - 1)];
                s.aug[r * lda + j] = x;
            });
            wsync();
            if (wave_gauss_jordan<false>(s.aug, lda, m, s.width, s.fac, s.prow)) status |= TFMPC_ST_NOT_PD;
            wave_for_2d(m, n, [&](int r, int j, int idx) {
                const S x = -s.aug[r * lda + m + 1 + j];
                s.K[r * ldn + j] = x;
                Kg[(size_t)t * m * n + idx] = x;
            });
            for (int r = lane; r < m; r += kWave) {
                const S x = -s.aug[r * lda + m];
                s.k[r] = x;
                kg[(size_t)t * m + r] = x;
            }
            wsync();
            // V' = Q_xx + Q_xu K (over Q_xx when folded) ; v' = q_x + Q_xu k  (Schur form; equal to lqr.py:97-105 in exact
            // arithmetic)
            P::matmul(n, n, m,
                        [&](int i, int k) { return s.Q[i * ldd + n + k]; },
                        [&](int k, int j) { return s.K[k * ldn + j]; },
                        [&](int i, int j) { return s.Q[i * ldd + j]; },
                        [&](int i, int j, S x) { s.Vn[i * ldv + j] = x; });
            for (int i = lane; i < n; i += kWave) {
                S s1 = S(0);
                for (int k = 0; k < m; ++k) s1 = fma(s.Q[i * ldd + n + k], s.k[k], s1);
                s.vn[i] = s.q[i] + s1;
            }
            // const += 1/2 k^T Q_uu k + k^T q_u + 1/2 f_t^T V f_t + f_t^T v (V, v before this step's update)
            S part = S(0);
            for (int r = lane; r < m; r += kWave) {
                S quk = S(0);
                for (int k = 0; k < m; ++k) quk = fma(s.Q[(n + r) * ldd + n + k], s.k[k], quk);
                part += s.k[r] * (S(0.5) * quk + s.q[n + r]);
            }
            for (int i = lane; i < n; i += kWave) {
                S vf = S(0);
                for (int k = 0; k < n; ++k) vf = fma(s.V[i * ldn + k], s.f[k], vf);
                part += s.f[i] * (S(0.5) * vf + s.v[i]);
            }
            cst += wave_sum(part);
            wsync();
            // V <- (V' + V'^T) / 2: the elimination above reads a symmetric Q_uu only while V stays symmetric
            wave_for_2d(n, n, [&](int i, int j, int idx) {
                const S x = S(0.5) * (s.Vn[i * ldv + j] + s.Vn[j * ldv + i]);
                s.V[i * ldn + j] = x;
                if (a.V) a.V[((size_t)b * Th + at(t)) * n * n + idx] = x;
            });
            for (int i = lane; i < n; i += kWave) {
                const S x = s.vn[i];
                s.v[i] = x;
                if (a.v) a.v[((size_t)b * Th + at(t)) * n + i] = x;
            }
            if (a.cst && lane == 0) a.cst[(size_t)b * Th + at(t)] = cst;
            wsync();
        }
        if (!P::valid(cst)) status |= TFMPC_ST_NAN;
    }

    if (FORWARD) {
        S *xs = a.states + (size_t)b * (Th + 1) * n;
        S *us = a.actions + (size_t)b * Th * m;
        S *cs = a.costs + (size_t)b * (Th + 1);
        if constexpr (SEG::kSegment) {
            xs += (size_t)seg.t0 * n;
            us += (size_t)seg.t0 * m;
            cs += seg.t0;
        }
        __syncthreads();                                 // gains written above are visible
        for (int i = lane; i < n; i += kWave) {
            S x;
            if constexpr (SEG::kSegment) x = seg.xstart[i];
            else x = a.x0[(size_t)b * n + i];
            s.z[i] = x;
            xs[i] = x;
        }
        for (int t = 0; t < T; ++t) {
            load_model(t);
            load_matrix(s.K, ldn, Kg + (size_t)t * m * n, m, n);
            for (int r = lane; r < m; r += kWave) s.k[r] = kg[(size_t)t * m + r];
            wsync();
            for (int r = lane; r < m; r += kWave) {        // u = K_t x + k_t
                S u = s.k[r];
                for (int j = 0; j < n; ++j) u = fma(s.K[r * ldn + j], s.z[j], u);
                s.z[n + r] = u;
                us[(size_t)t * m + r] = u;
            }
            wsync();
            S part = S(0);                                 // 1/2 z^T C_t z + c_t^T z
            for (int r = lane; r < d; r += kWave) {
                S cz = S(0);
                for (int j = 0; j < d; ++j) cz = fma(s.C[r * ldd + j], s.z[j], cz);
                part += s.z[r] * (S(0.5) * cz + s.c[r]);
            }
            for (int i = lane; i < n; i += kWave) {        // x' = F_t z + f_t
                S x = s.f[i];
                for (int j = 0; j < d; ++j) x = fma(s.F[i * ldd + j], s.z[j], x);
                s.xn[i] = x;
            }
            const S cost = wave_sum(part);
            if (lane == 0) cs[t] = cost;
            wsync();
            for (int i = lane; i < n; i += kWave) {
                const S x = s.xn[i];
                s.z[i] = x;
                if constexpr (SEG::kSegment) {               // (the next segment writes its own first state)
                    if (seg.last || t + 1 < T) xs[(size_t)(t + 1) * n + i] = x;
                } else {
                    xs[(size_t)(t + 1) * n + i] = x;
                }
            }
            wsync();
        }
        bool last = true;
        if constexpr (SEG::kSegment) last = seg.last;
        if (last) {
            S part = S(0);                                 // 1/2 x^T C_fin x + c_fin^T x
            for (int r = lane; r < n; r += kWave) {
                S cz = S(0);
                for (int j = 0; j < n; ++j) cz = fma(Cf[r * ldf + j], s.z[j], cz);
                part += s.z[r] * (S(0.5) * cz + cf[r]);
            }
            const S last_cost = wave_sum(part);
            if (lane == 0) cs[T] = last_cost;
            if (!P::valid(last_cost)) status |= TFMPC_ST_NAN;
        }
    }

    if constexpr (SEG::kSegment) {
        if (lane == 0) *seg.status = status;
    } else {
        if (a.status && lane == 0) a.status[b] = status;
    }
}

// One launch of a wave-per-instance kernel with `smem` bytes of dynamic LDS per wave.
template <class S>
int tv_wave_launch(void (*kern)(TvLqrArgsT<S>), const TvLqrArgsT<S> &a, size_t smem, hipStream_t stream)
{
    return launch_with_lds(kern, a.B, kWave, smem, stream, a);
}

}  // namespace tfmpc
