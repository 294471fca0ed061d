// tvlqr_kernels.h -- internal launch interface of the time-varying LQR kernels (tvlqr_mfma16x8.hip; tvlqr_generic.hip
// and tvlqr_f64.hip, the fp32 and double instantiations of tvlqr_wave.h's one body) and their C-ABI dispatcher
// (tvlqr_dispatch.hip, both precisions).  Not installed; the public contract is the TV-LQR block of
// include/tfmpc_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/tfmpc_hip.h"

namespace tfmpc {

// Model operand X of instance b at step t starts at X + b * sX_b + t * sX_t (elements; 0 = shared / constant).
template <class S>
struct TvLqrArgsT {
    int B, n, m, T;
    const S *F, *f, *C, *c;
    long sF_b, sF_t, sf_b, sf_t, sC_b, sC_t, sc_b, sc_t;
    const S *Cfin, *cfin;         // final cost [n][n], [n]; both NULL: C_{T-1}[:n,:n], c_{T-1}[:n]
    long sCfin_b, scfin_b;
    const S *x0;
    S *K, *k;                     // [B][T][m][n], [B][T][m]
    long sK, sk;                  // batch strides of K, k (forward-only launches may share a policy: 0)
    S *V, *v, *cst;               // optional value-function outputs [B][T][n][n], [B][T][n], [B][T]
    S *states, *actions, *costs;
    int32_t *status;
    const uint32_t *mask;         // [B][T] or NULL; bit i: control i is held at step t (masked sweep)
};
using TvLqrArgs = TvLqrArgsT<float>;

template <class S>
__host__ __device__ inline const S *tv_at(const S *p, long sb, long st, int b, int t)
{
    return p + (size_t)b * sb + (size_t)t * st;
}

bool tvlqr_mfma_supported(int n, int m);
int tvlqr_mfma_launch(const TvLqrArgs &a, bool backward, bool forward, hipStream_t stream);

size_t tvlqr_generic_smem_bytes(int n, int m);
int tvlqr_generic_launch(const TvLqrArgs &a, bool backward, bool forward, hipStream_t stream);

// double precision: n <= 32 and m <= 32; the name is "tv_f64_wave16" or "tv_f64_wave32"
bool tvlqr_f64_supported(int n, int m);
const char *tvlqr_f64_kernel_name(int n, int m);
int tvlqr_f64_launch(const TvLqrArgsT<double> &a, bool backward, bool forward, hipStream_t stream);

// The time-parallel double solve (tfmpc_tvlqr_solve_time_parallel_f64): the horizon in `segments`
// pieces of `len` steps (the last one shorter), one wave per (instance, segment), w = b * segments + i.
struct TvTimeParallel {
    int segments, len;
    double *elems;                // [B segments][3 n n + 2 n]: A, G, H, b, h of the condensed segment
    double *Vend, *vend;          // [B segments][n][n], [n]: the value function at the segment's end
    double *xstart;               // [B segments][n]: the state at the segment's start
    int32_t *st_condense, *st_stitch, *st_expand;     // [B segments], [B], [B segments]
};
__host__ __device__ constexpr size_t tv_tp_elem_doubles(int n) { return (size_t)3 * n * n + 2 * n; }

const char *tvlqr_time_parallel_f64_kernel_name(int n, int m);
// condense + stitch (tvlqr_time_parallel_f64.hip), expand (tvlqr_f64.hip: the body of tvlqr_wave.h on a segment), then
// the status OR and the NaN fill of flagged instances (every non-NULL output of a); a.cst is NULL
int tvlqr_time_parallel_f64_condense_launch(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, hipStream_t stream);
int tvlqr_time_parallel_f64_stitch_launch(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, hipStream_t stream);
int tvlqr_f64_expand_launch(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, hipStream_t stream);
int tvlqr_time_parallel_f64_finish_launch(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, hipStream_t stream);

// The periodic infinite-horizon LQR in double (tfmpc_tvlqr_periodic_steady_state_f64): a.T is ONE PERIOD,
// cut into tp.segments pieces as the time-parallel solve cuts a horizon (tp.xstart is not used); a.Cfin, a.x0 and the
// rollout's outputs are NULL.
struct TvPeriodic {
    int max_iter;
    double tol;
    double *E1;                   // [B][3 n n + 2 n]: the one-period element
    double *residual;             // [B] or NULL
    int32_t *iterations;          // [B] or NULL
};
const char *tvlqr_periodic_f64_kernel_name(int n, int m);
// condense (the time-parallel solve's own launch), periodic stitch (tvlqr_periodic_f64.hip), expand without a rollout
// (tvlqr_f64.hip; a.K and a.k are written, the caller's or scratch), then the status OR and the NaN fill of flagged
// instances (every non-NULL of a.K, a.k, a.V, a.v and pp.residual; a.status is required)
int tvlqr_periodic_f64_stitch_launch(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, const TvPeriodic &pp,
                                     hipStream_t stream);
int tvlqr_f64_periodic_expand_launch(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, hipStream_t stream);
int tvlqr_periodic_f64_finish_launch(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, const TvPeriodic &pp,
                                     hipStream_t stream);

// tfmpc_tvlqr_solve_f32 (same arguments, K = k = V = v = cst = NULL) on a MASKED model: for every set bit i of
// mask[b][t], column n + i of F_t is read as zero, row and column n + i of C_t as zero with a unit diagonal, and
// entry n + i of c_t as zero, so that row i of K_t and k_t[i] are exactly zero.  The mask is applied as the operands
// are loaded; no masked copy of the model exists.  m <= 32.  mask == NULL is the plain solve.
int tvlqr_solve_masked_f32(int B, int n, int m, int T, const float *F, long sF_b, long sF_t, const float *f, long sf_b,
                           long sf_t, const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t,
                           const float *Cfin, long sCfin_b, const float *cfin, long scfin_b, const float *x0,
                           float *states, float *actions, float *costs, int32_t *status, const uint32_t *mask,
                           void *workspace, size_t workspace_bytes, void *stream);

// The same in double, n <= 32 and m <= 32, which also hands out the masked problem's value function:
// V[B][T][n][n], v[B][T][n] (each optional).  states == NULL runs the backward sweep alone (x0, actions, costs are then
// not read or written).  The gains go to the workspace, tfmpc_tvlqr_workspace_bytes_f64.  The kernel's name is
// "tv_masked_f64_wave16" or "tv_masked_f64_wave32".
const char *tvlqr_f64_masked_kernel_name(int n, int m);
int tvlqr_f64_masked_launch(const TvLqrArgsT<double> &a, bool forward, hipStream_t stream);
int tvlqr_solve_masked_f64(int B, int n, int m, int T, const double *F, long sF_b, long sF_t, const double *f, long sf_b,
                           long sf_t, const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                           const double *Cfin, long sCfin_b, const double *cfin, long scfin_b, const double *x0,
                           double *states, double *actions, double *costs, double *V, double *v, int32_t *status,
                           const uint32_t *mask, void *workspace, size_t workspace_bytes, void *stream);

}  // namespace tfmpc
