// tvlqr_box_wave.h -- arguments, policy contract and entry point of the control-limited TIME-VARYING LQR forward solve
// (DESIGN.md 3.17, 3.18); the kernels' one body is tvlqr_box_body.h, included in each kernel.  The problem:
//   min sum_t 1/2 z_t^T C_t z_t + c_t^T z_t + final cost,  x_{t+1} = F_t z_t + f_t,  low_t <= u_t <= high_t,
// a convex QP with an exact model, solved by control-limited Newton sweeps WITHOUT regularisation.  One wavefront per
// instance, the unfolded LDS layout and per-step model copy of tvlqr_wave.h, instantiated in fp32 by tvlqr_box.hip
// (tfmpc_tvlqr_box_solve_f32) and in double by tvlqr_box_f64.hip (tfmpc_tvlqr_box_solve_f64).
//
// Per pass: a backward sweep in delta form around the nominal (x, u) -- Q = C_t + F_t^T V F_t, q = C_t z_t + c_t +
// F_t^T v, a box-QP in du by projected Newton (lane r owns control r; the free block is eliminated without pivoting from
// the augmented [Q_uu | g | Q_ux] with held rows and columns replaced by identity, so ONE elimination gives the Newton
// step and the gains K_f), V <- sym(Q_xx + Q_xu K), v <- q_x + Q_xu k -- then a line search over eleven step sizes, each
// a clipped closed-loop rollout into the workspace; the accepted candidate is copied into the output arrays, which hold
// the nominal.  The sweep that meets the stop rule still has its step applied (in full, untested): a step of tol left out
// is several roundings of the optimum.  Instances never talk to each other: no atomics, no waits, every loop has a
// fixed bound, and every branch around a fence is taken on a wave-uniform value (a reduction, a ballot or a broadcast).
//
// A policy P carries what differs between the precisions and nothing else:
//   P::T, P::matmul                       the scalar type and the matrix-core product: WaveF32 or WaveF64<MAXD> (wave_ops_f64.h)
//   P::kArmijo, kTrustRatio, kDefaultTol  the constants in P::T (tol = 0 selects kDefaultTol: 4e-6 in fp32, 1e-12 in double)
// The LDS layout is the unfolded one in both: the box-QP keeps its gradient in s.prow, and q is formed from s.C after
// the product that writes s.Q, so tvlqr_wave.h's folded layout (Q over C_t, no prow) does not serve this body.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <limits>

#include "tvlqr_wave.h"

namespace tfmpc {

constexpr int kQpIterations = 100, kQpBacktracks = 21, kAlphas = 11, kTrustedInARow = 3;
constexpr int kDefaultPasses = 100;
constexpr int kReasonConverged = 0, kReasonNoDecrease = 1, kReasonPassCap = 2, kReasonFailed = 3;

template <class S>
struct TvBoxArgsT {
    TvLqrArgsT<S> a;                // model, x0; K, k: the gains (workspace); states, actions, costs: the nominal
    const S *low, *high;            // [m] per (b, t)
    long slow_b, slow_t, shigh_b, shigh_t;
    const S *u_init;                // [T][m] per instance (batch stride su_b) or NULL: zeros
    long su_b;
    int max_iter;
    S tol;
    S *cx, *cu, *cc;                // the candidate trajectory [B][T+1][n], [B][T][m], [B][T+1] (workspace)
    int32_t *iterations, *reason;
    uint32_t *clamp_mask;           // [B][T] or NULL
};

// gains K, k and the candidate trajectory, in elements
inline size_t tv_box_workspace_elems(int B, int n, int m, int T)
{
    return (size_t)B * ((size_t)T * m * (n + 1) + ((size_t)T + 1) * n + (size_t)T * m + ((size_t)T + 1));
}

// The entry point behind tfmpc_tvlqr_box_solve_f32 / _f64: argument, shape and workspace checks in that order, then one
// launch of `kern` (one wave per instance, the unfolded layout's LDS).
template <class S>
int tv_box_solve(void (*kern)(TvBoxArgsT<S>), bool supported, int B, int n, int m, int T, const S *F, long sF_b, long sF_t,
                 const S *f, long sf_b, long sf_t, const S *C, long sC_b, long sC_t, const S *c, long sc_b, long sc_t,
                 const S *Cfin, long sCfin_b, const S *cfin, long scfin_b, const S *low, long slow_b, long slow_t,
                 const S *high, long shigh_b, long shigh_t, const S *x0, const S *u_init, long su_b, int max_iter, S tol,
                 S *states, S *actions, S *costs, int32_t *iterations, int32_t *status, int32_t *reason,
                 uint32_t *clamp_mask, void *workspace, size_t workspace_bytes, void *stream)
{
    if (B < 0 || n <= 0 || m <= 0 || T <= 0 || max_iter < 0 || !(tol >= S(0))) return TFMPC_ERR_ARG;
    if (!supported) return TFMPC_ERR_UNSUPPORTED;
    if (B == 0) return TFMPC_OK;                                    // no-op: nothing is read
    if (!F || !f || !C || !c || !low || !high || !x0) return TFMPC_ERR_ARG;
    if (!Cfin != !cfin) return TFMPC_ERR_ARG;                       // both or neither
    for (long s : {sF_b, sF_t, sf_b, sf_t, sC_b, sC_t, sc_b, sc_t, sCfin_b, scfin_b, slow_b, slow_t, shigh_b, shigh_t, su_b})
        if (s < 0) return TFMPC_ERR_ARG;
    if (!states || !actions || !costs || !iterations || !status) return TFMPC_ERR_ARG;
    if (!workspace || workspace_bytes < tv_box_workspace_elems(B, n, m, T) * sizeof(S)) return TFMPC_ERR_WORKSPACE;

    TvBoxArgsT<S> p{};
    TvLqrArgsT<S> &a = p.a;
    a.B = B; a.n = n; a.m = m; a.T = T;
    a.F = F; a.sF_b = sF_b; a.sF_t = sF_t;
    a.f = f; a.sf_b = sf_b; a.sf_t = sf_t;
    a.C = C; a.sC_b = sC_b; a.sC_t = sC_t;
    a.c = c; a.sc_b = sc_b; a.sc_t = sc_t;
    a.Cfin = Cfin; a.sCfin_b = sCfin_b;
    a.cfin = cfin; a.scfin_b = scfin_b;
    a.x0 = x0;
    S *w = static_cast<S *>(workspace);
    a.K = w; a.sK = (long)T * m * n; w += (size_t)B * T * m * n;
    a.k = w; a.sk = (long)T * m; w += (size_t)B * T * m;
    p.cx = w; w += (size_t)B * ((size_t)T + 1) * n;
    p.cu = w; w += (size_t)B * T * m;
    p.cc = w;
    a.states = states; a.actions = actions; a.costs = costs; a.status = status;
    p.low = low; p.slow_b = slow_b; p.slow_t = slow_t;
    p.high = high; p.shigh_b = shigh_b; p.shigh_t = shigh_t;
    p.u_init = u_init; p.su_b = su_b;
    p.max_iter = max_iter; p.tol = tol;
    p.iterations = iterations; p.reason = reason; p.clamp_mask = clamp_mask;

    const size_t smem = tv_smem_elems<false>(n, m) * sizeof(S);
    return launch_with_lds(kern, B, kWave, smem, static_cast<hipStream_t>(stream), p);      // (`supported` bounds smem)
}

}  // namespace tfmpc
