// tvlqr_dispatch.hip -- extern "C" entry points of the time-varying LQR (include/tfmpc_hip.h, TV-LQR block), fp32 and
// double: argument checks, kernel-variant choice, launch.  No allocation, no sync.  Both precisions run the same
// checks in the same order; only the support test and the launcher differ.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "lqr_kernels.h"
#include "options.h"
#include "tvlqr_kernels.h"

using namespace tfmpc;

namespace {

template <class S>
struct Model {
    const S *F; long sF_b, sF_t;
    const S *f; long sf_b, sf_t;
    const S *C; long sC_b, sC_t;
    const S *c; long sc_b, sc_t;
    const S *Cfin; long sCfin_b;
    const S *cfin; long scfin_b;
};

bool supported(float, int n, int m) { return tvlqr_mfma_supported(n, m) || tvlqr_generic_smem_bytes(n, m) <= kMaxLdsBytes; }
bool supported(double, int n, int m) { return tvlqr_f64_supported(n, m); }

int launch(const TvLqrArgsT<float> &a, bool bw, bool fw, hipStream_t s)
{
    return tvlqr_mfma_supported(a.n, a.m) ? tvlqr_mfma_launch(a, bw, fw, s) : tvlqr_generic_launch(a, bw, fw, s);
}
int launch(const TvLqrArgsT<double> &a, bool bw, bool fw, hipStream_t s) { return tvlqr_f64_launch(a, bw, fw, s); }

template <class S>
int check_model(int B, int n, int m, int T, const Model<S> &md)
{
    if (B < 0 || n <= 0 || m <= 0 || T <= 0) return TFMPC_ERR_ARG;
    if (!supported(S(), n, m)) return TFMPC_ERR_UNSUPPORTED;
    if (B == 0) return TFMPC_OK;                                    // no-op: nothing is read (empty tensors may be NULL)
    if (!md.F || !md.f || !md.C || !md.c) return TFMPC_ERR_ARG;
    if (!md.Cfin != !md.cfin) return TFMPC_ERR_ARG;                 // both or neither
    for (long s : {md.sF_b, md.sF_t, md.sf_b, md.sf_t, md.sC_b, md.sC_t, md.sc_b, md.sc_t, md.sCfin_b, md.scfin_b})
        if (s < 0) return TFMPC_ERR_ARG;
    return TFMPC_OK;
}

template <class S>
TvLqrArgsT<S> make_args(int B, int n, int m, int T, const Model<S> &md)
{
    TvLqrArgsT<S> a{};
    a.B = B; a.n = n; a.m = m; a.T = T;
    a.F = md.F; a.sF_b = md.sF_b; a.sF_t = md.sF_t;
    a.f = md.f; a.sf_b = md.sf_b; a.sf_t = md.sf_t;
    a.C = md.C; a.sC_b = md.sC_b; a.sC_t = md.sC_t;
    a.c = md.c; a.sc_b = md.sc_b; a.sc_t = md.sc_t;
    a.Cfin = md.Cfin; a.sCfin_b = md.sCfin_b;
    a.cfin = md.cfin; a.scfin_b = md.scfin_b;
    return a;
}

template <class S>
size_t workspace_bytes(int B, int n, int m, int T)
{
    if (B <= 0 || n <= 0 || m <= 0 || T <= 0) return 0;
    return (size_t)B * T * m * (n + 1) * sizeof(S);
}

template <class S>
int backward(int B, int n, int m, int T, const Model<S> &md, S *K, S *k, S *V, S *v, S *cst, int32_t *status, void *stream)
{
    int rc = check_model(B, n, m, T, md);
    if (rc != TFMPC_OK || B == 0) return rc;
    if (!K || !k) return TFMPC_ERR_ARG;
    TvLqrArgsT<S> a = make_args(B, n, m, T, md);
    a.K = K; a.k = k; a.sK = (long)T * m * n; a.sk = (long)T * m;
    a.V = V; a.v = v; a.cst = cst; a.status = status;
    return launch(a, true, false, static_cast<hipStream_t>(stream));
}

template <class S>
int forward(int B, int n, int m, int T, const Model<S> &md, const S *K, long strideK, const S *k, long stride_k,
            const S *x0, S *states, S *actions, S *costs, void *stream)
{
    int rc = check_model(B, n, m, T, md);
    if (rc != TFMPC_OK || B == 0) return rc;
    if (strideK < 0 || stride_k < 0) return TFMPC_ERR_ARG;
    if (!x0 || !states || !costs || !K || !k || !actions) return TFMPC_ERR_ARG;
    TvLqrArgsT<S> a = make_args(B, n, m, T, md);
    a.x0 = x0;
    a.K = const_cast<S *>(K); a.k = const_cast<S *>(k); a.sK = strideK; a.sk = stride_k;
    a.states = states; a.actions = actions; a.costs = costs;
    return launch(a, false, true, static_cast<hipStream_t>(stream));
}

// mask != NULL: the masked sweep (fp32: tvlqr_solve_masked_f32; double has its own entry, tvlqr_solve_masked_f64)
template <class S>
int solve(int B, int n, int m, int T, const Model<S> &md, const S *x0, S *states, S *actions, S *costs, S *K, S *k,
          S *V, S *v, S *cst, int32_t *status, const uint32_t *mask, void *workspace, size_t workspace_bytes_given,
          void *stream)
{
    int rc = check_model(B, n, m, T, md);
    if (rc != TFMPC_OK || B == 0) return rc;
    if (!x0 || !states || !costs || !actions) return TFMPC_ERR_ARG;
    if (mask && m > 32) return TFMPC_ERR_UNSUPPORTED;
    if (!K || !k) {
        // gains are not a requested output: keep them in caller-provided scratch
        if (!workspace || workspace_bytes_given < workspace_bytes<S>(B, n, m, T)) return TFMPC_ERR_WORKSPACE;
        S *w = static_cast<S *>(workspace);
        if (!K) K = w;
        if (!k) k = w + (size_t)B * T * m * n;
    }
    TvLqrArgsT<S> a = make_args(B, n, m, T, md);
    a.x0 = x0;
    a.K = K; a.k = k; a.sK = (long)T * m * n; a.sk = (long)T * m;
    a.V = V; a.v = v; a.cst = cst;
    a.states = states; a.actions = actions; a.costs = costs; a.status = status;
    a.mask = mask;
    return launch(a, true, true, static_cast<hipStream_t>(stream));
}

// The time-parallel solve's segment table: `segments` clamped to T, every segment len = ceil(T / segments) steps but a
// shorter last one, count = ceil(T / len) of them.
struct SegmentTable {
    int len, count;
};
SegmentTable segment_table(int T, int segments)
{
    if (segments > T) segments = T;
    const long len = ((long)T + segments - 1) / segments;
    return {(int)len, (int)((T + len - 1) / len)};
}

size_t up8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

// doubles: the elements, the value function and the state at every segment boundary, the gains; then the status words
size_t time_parallel_workspace_bytes(int B, int n, int m, int T, int segments)
{
    if (B <= 0 || n <= 0 || m <= 0 || T <= 0 || segments < 1) return 0;
    const size_t w = (size_t)B * segment_table(T, segments).count;
    return sizeof(double) * (w * (tv_tp_elem_doubles(n) + (size_t)n * n + 2 * n) + (size_t)B * T * m * (n + 1)) +
           up8(sizeof(int32_t) * (2 * w + B));
}

// doubles: the segment elements and the one-period elements, the value function at every segment's end, the gains; then
// the status words
size_t periodic_workspace_bytes(int B, int n, int m, int N, int segments)
{
    if (B <= 0 || n <= 0 || m <= 0 || N <= 0 || segments < 1) return 0;
    const size_t w = (size_t)B * segment_table(N, segments).count;
    return sizeof(double) * ((w + B) * tv_tp_elem_doubles(n) + w * ((size_t)n * n + n) + (size_t)B * N * m * (n + 1)) +
           up8(sizeof(int32_t) * (2 * w + B));
}

constexpr int kPeriodicMaxIter = 40;                     // DESIGN.md 3.16's defaults
constexpr double kPeriodicTol = 4.0 * DBL_EPSILON;

}  // namespace

#define TFMPC_TVLQR_MODEL_PARAMS(S)                                                                                    \
    int B, int n, int m, int T, const S *F, long sF_b, long sF_t, const S *f, long sf_b, long sf_t, const S *C, long sC_b, \
        long sC_t, const S *c, long sc_b, long sc_t, const S *Cfin, long sCfin_b, const S *cfin, long scfin_b
#define TFMPC_TVLQR_MODEL(S) \
    B, n, m, T, Model<S>{F, sF_b, sF_t, f, sf_b, sf_t, C, sC_b, sC_t, c, sc_b, sc_t, Cfin, sCfin_b, cfin, scfin_b}

namespace tfmpc {

int tvlqr_solve_masked_f32(TFMPC_TVLQR_MODEL_PARAMS(float), const float *x0, float *states, float *actions, float *costs,
                           int32_t *status, const uint32_t *mask, void *workspace, size_t workspace_bytes, void *stream)
{
    return solve<float>(TFMPC_TVLQR_MODEL(float), x0, states, actions, costs, nullptr, nullptr, nullptr, nullptr, nullptr,
                        status, mask, workspace, workspace_bytes, stream);
}

int tvlqr_solve_masked_f64(TFMPC_TVLQR_MODEL_PARAMS(double), const double *x0, double *states, double *actions,
                           double *costs, double *V, double *v, int32_t *status, const uint32_t *mask, void *workspace,
                           size_t workspace_bytes_given, void *stream)
{
    const Model<double> md{F, sF_b, sF_t, f, sf_b, sf_t, C, sC_b, sC_t, c, sc_b, sc_t, Cfin, sCfin_b, cfin, scfin_b};
    int rc = check_model(B, n, m, T, md);
    if (rc != TFMPC_OK || B == 0) return rc;
    const bool forward = states != nullptr;
    if (!mask || (forward && (!x0 || !actions || !costs))) return TFMPC_ERR_ARG;
    if (!workspace || workspace_bytes_given < workspace_bytes<double>(B, n, m, T)) return TFMPC_ERR_WORKSPACE;
    double *w = static_cast<double *>(workspace);
    TvLqrArgsT<double> a = make_args(B, n, m, T, md);
    a.x0 = x0;
    a.K = w; a.k = w + (size_t)B * T * m * n; a.sK = (long)T * m * n; a.sk = (long)T * m;
    a.V = V; a.v = v;
    a.states = states; a.actions = actions; a.costs = costs; a.status = status;
    a.mask = mask;
    return tvlqr_f64_masked_launch(a, forward, static_cast<hipStream_t>(stream));
}

}  // namespace tfmpc

extern "C" {

size_t tfmpc_tvlqr_workspace_bytes(int B, int n, int m, int T) { return workspace_bytes<float>(B, n, m, T); }
size_t tfmpc_tvlqr_workspace_bytes_f64(int B, int n, int m, int T) { return workspace_bytes<double>(B, n, m, T); }

const char *tfmpc_tvlqr_kernel_name(int n, int m, int T)
{
    (void)T;
    if (n <= 0 || m <= 0) return "invalid";
    if (tvlqr_mfma_supported(n, m)) return (n == 16 && m == 8) ? "tv_mfma_16x8" : "tv_mfma_16x8 (zero-padded)";
    if (!supported(float(), n, m)) return "unsupported";
    return "tv_generic_wave";
}

const char *tfmpc_tvlqr_kernel_name_f64(int n, int m, int T)
{
    (void)T;
    if (n <= 0 || m <= 0) return "invalid";
    if (!supported(double(), n, m)) return "unsupported";
    return tvlqr_f64_kernel_name(n, m);
}

int tfmpc_tvlqr_backward_f32(TFMPC_TVLQR_MODEL_PARAMS(float), float *K, float *k, float *V, float *v, float *cst,
                             int32_t *status, void *stream)
{
    return backward<float>(TFMPC_TVLQR_MODEL(float), K, k, V, v, cst, status, stream);
}

int tfmpc_tvlqr_backward_f64(TFMPC_TVLQR_MODEL_PARAMS(double), double *K, double *k, double *V, double *v, double *cst,
                             int32_t *status, void *stream)
{
    return backward<double>(TFMPC_TVLQR_MODEL(double), K, k, V, v, cst, status, stream);
}

int tfmpc_tvlqr_forward_f32(TFMPC_TVLQR_MODEL_PARAMS(float), const float *K, long strideK, const float *k, long stride_k,
                            const float *x0, float *states, float *actions, float *costs, void *stream)
{
    return forward<float>(TFMPC_TVLQR_MODEL(float), K, strideK, k, stride_k, x0, states, actions, costs, stream);
}

int tfmpc_tvlqr_forward_f64(TFMPC_TVLQR_MODEL_PARAMS(double), const double *K, long strideK, const double *k,
                            long stride_k, const double *x0, double *states, double *actions, double *costs, void *stream)
{
    return forward<double>(TFMPC_TVLQR_MODEL(double), K, strideK, k, stride_k, x0, states, actions, costs, stream);
}

int tfmpc_tvlqr_solve_f32(TFMPC_TVLQR_MODEL_PARAMS(float), const float *x0, float *states, float *actions, float *costs,
                          float *K, float *k, float *V, float *v, float *cst, int32_t *status,
                          void *workspace, size_t workspace_bytes, void *stream)
{
    return solve<float>(TFMPC_TVLQR_MODEL(float), x0, states, actions, costs, K, k, V, v, cst, status, nullptr, workspace,
                        workspace_bytes, stream);
}

int tfmpc_tvlqr_solve_f64(TFMPC_TVLQR_MODEL_PARAMS(double), const double *x0, double *states, double *actions,
                          double *costs, double *K, double *k, double *V, double *v, double *cst, int32_t *status,
                          void *workspace, size_t workspace_bytes, void *stream)
{
    return solve<double>(TFMPC_TVLQR_MODEL(double), x0, states, actions, costs, K, k, V, v, cst, status, nullptr,
                         workspace, workspace_bytes, stream);
}

size_t tfmpc_tvlqr_time_parallel_workspace_bytes_f64(int B, int n, int m, int T, int segments)
{
    return time_parallel_workspace_bytes(B, n, m, T, segments);
}

const char *tfmpc_tvlqr_time_parallel_kernel_name_f64(int n, int m, int T, int segments)
{
    if (n <= 0 || m <= 0 || T <= 0 || segments < 1) return "invalid";
    if (!supported(double(), n, m)) return "unsupported";
    return segment_table(T, segments).count == 1 ? tvlqr_f64_kernel_name(n, m) : tvlqr_time_parallel_f64_kernel_name(n, m);
}

int tfmpc_tvlqr_solve_time_parallel_f64(TFMPC_TVLQR_MODEL_PARAMS(double), const double *x0, double *states,
                                        double *actions, double *costs, double *K, double *k, double *V, double *v,
                                        double *cst, int32_t *status, int segments, void *workspace,
                                        size_t workspace_bytes, void *stream)
{
    const Model<double> md{F, sF_b, sF_t, f, sf_b, sf_t, C, sC_b, sC_t, c, sc_b, sc_t, Cfin, sCfin_b, cfin, scfin_b};
    int rc = check_model(B, n, m, T, md);
    if (rc != TFMPC_OK) return rc;
    if (segments < 1 || cst) return TFMPC_ERR_ARG;           // the constant term is not carried through the elements
    if (B == 0) return TFMPC_OK;
    if (!x0 || !states || !costs || !actions) return TFMPC_ERR_ARG;
    const SegmentTable tab = segment_table(T, segments);
    if (tab.count == 1)
        return solve<double>(B, n, m, T, md, x0, states, actions, costs, K, k, V, v, nullptr, status, nullptr, workspace,
                             workspace_bytes, stream);
    const size_t waves = (size_t)B * tab.count;
    if (waves > (size_t)INT32_MAX) return TFMPC_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < time_parallel_workspace_bytes(B, n, m, T, segments)) return TFMPC_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) % sizeof(double)) return TFMPC_ERR_ARG;      // doubles are carved from it
    TvTimeParallel tp{};
    tp.segments = tab.count;
    tp.len = tab.len;
    double *w = static_cast<double *>(workspace);
    tp.elems = w; w += waves * tv_tp_elem_doubles(n);
    tp.Vend = w; w += waves * n * n;
    tp.vend = w; w += waves * n;
    tp.xstart = w; w += waves * n;
    double *gains = w; w += (size_t)B * T * m * (n + 1);
    int32_t *st = reinterpret_cast<int32_t *>(w);
    tp.st_condense = st;
    tp.st_expand = st + waves;
    tp.st_stitch = st + 2 * waves;
    TvLqrArgsT<double> a = make_args(B, n, m, T, md);
    a.x0 = x0;
    a.K = K ? K : gains;
    a.k = k ? k : gains + (size_t)B * T * m * n;
    a.sK = (long)T * m * n; a.sk = (long)T * m;
    a.V = V; a.v = v;
    a.states = states; a.actions = actions; a.costs = costs; a.status = status;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // TFMPC_TVLQR_TP_PHASES=1|2: stop after the condense / the stitch launch -- for the phase split of
    // tools/tvlqr_time_parallel_rate.py only; no output is written, and the call says so: TFMPC_TVLQR_TP_STOPPED, not OK
    const int phases = option_int(kOptTvlqrTpPhases, 3);
    if ((rc = tvlqr_time_parallel_f64_condense_launch(a, tp, s)) != TFMPC_OK) return rc;
    if (phases == 1) return TFMPC_TVLQR_TP_STOPPED;
    if ((rc = tvlqr_time_parallel_f64_stitch_launch(a, tp, s)) != TFMPC_OK) return rc;
    if (phases == 2) return TFMPC_TVLQR_TP_STOPPED;
    if ((rc = tvlqr_f64_expand_launch(a, tp, s)) != TFMPC_OK) return rc;
    if (!K) a.K = nullptr;                                   // scratch gains are nobody's output
    if (!k) a.k = nullptr;
    return tvlqr_time_parallel_f64_finish_launch(a, tp, s);
}

size_t tfmpc_tvlqr_periodic_workspace_bytes_f64(int B, int n, int m, int N, int segments)
{
    return periodic_workspace_bytes(B, n, m, N, segments);
}

const char *tfmpc_tvlqr_periodic_kernel_name_f64(int n, int m, int N, int segments)
{
    if (n <= 0 || m <= 0 || N <= 0 || segments < 1) return "invalid";
    if (!supported(double(), n, m)) return "unsupported";
    return tvlqr_periodic_f64_kernel_name(n, m);
}

int tfmpc_tvlqr_periodic_steady_state_f64(int B, int n, int m, int N, const double *F, long sF_b, long sF_t,
                                          const double *f, long sf_b, long sf_t, const double *C, long sC_b, long sC_t,
                                          const double *c, long sc_b, long sc_t, int segments, int max_iter, double tol,
                                          double *K, double *k, double *V, double *v, double *residual,
                                          int32_t *iterations, int32_t *status, void *workspace, size_t workspace_bytes,
                                          void *stream)
{
    const Model<double> md{F, sF_b, sF_t, f, sf_b, sf_t, C, sC_b, sC_t, c, sc_b, sc_t, nullptr, 0, nullptr, 0};
    int rc = check_model(B, n, m, N, md);
    if (rc != TFMPC_OK) return rc;
    if (segments < 1 || max_iter < 0 || !(tol >= 0.0)) return TFMPC_ERR_ARG;
    if (B == 0) return TFMPC_OK;
    if (!status) return TFMPC_ERR_ARG;
    const SegmentTable tab = segment_table(N, segments);
    const size_t waves = (size_t)B * tab.count;
    if (waves > (size_t)INT32_MAX) return TFMPC_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < periodic_workspace_bytes(B, n, m, N, segments)) return TFMPC_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(workspace) % sizeof(double)) return TFMPC_ERR_ARG;      // doubles are carved from it
    TvTimeParallel tp{};
    tp.segments = tab.count;
    tp.len = tab.len;
    TvPeriodic pp{};
    pp.max_iter = max_iter ? max_iter : kPeriodicMaxIter;
    pp.tol = tol > 0.0 ? tol : kPeriodicTol;
    pp.residual = residual;
    pp.iterations = iterations;
    double *w = static_cast<double *>(workspace);
    tp.elems = w; w += waves * tv_tp_elem_doubles(n);
    pp.E1 = w; w += (size_t)B * tv_tp_elem_doubles(n);
    tp.Vend = w; w += waves * n * n;
    tp.vend = w; w += waves * n;
    double *gains = w; w += (size_t)B * N * m * (n + 1);
    int32_t *st = reinterpret_cast<int32_t *>(w);
    tp.st_condense = st;
    tp.st_expand = st + waves;
    tp.st_stitch = st + 2 * waves;
    TvLqrArgsT<double> a = make_args(B, n, m, N, md);
    a.K = K ? K : gains;
    a.k = k ? k : gains + (size_t)B * N * m * n;
    a.sK = (long)N * m * n; a.sk = (long)N * m;
    a.V = V; a.v = v;
    a.status = status;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // TFMPC_TVLQR_TP_PHASES=1|2|3: stop after the condense / the stitch / the expand launch, as the time-parallel solve
    // does -- for the phase split of tools/tvlqr_periodic_rate.py only: TFMPC_TVLQR_TP_STOPPED, not OK
    const int phases = option_int(kOptTvlqrTpPhases, 4);
    if ((rc = tvlqr_time_parallel_f64_condense_launch(a, tp, s)) != TFMPC_OK) return rc;
    if (phases == 1) return TFMPC_TVLQR_TP_STOPPED;
    if ((rc = tvlqr_periodic_f64_stitch_launch(a, tp, pp, s)) != TFMPC_OK) return rc;
    if (phases == 2) return TFMPC_TVLQR_TP_STOPPED;
    if ((rc = tvlqr_f64_periodic_expand_launch(a, tp, s)) != TFMPC_OK) return rc;
    if (phases == 3) return TFMPC_TVLQR_TP_STOPPED;
    if (!K) a.K = nullptr;                                   // scratch gains are nobody's output
    if (!k) a.k = nullptr;
    return tvlqr_periodic_f64_finish_launch(a, tp, pp, s);
}

}  // extern "C"
