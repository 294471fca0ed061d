// tvlqr_dispatch.hip -- extern "C" entry points of the time-varying LQR (include/tfmpc_hip.h, TV-LQR block):
// argument checks, kernel-variant choice, launch.  No allocation, no sync.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lqr_kernels.h"
#include "tvlqr_kernels.h"

using namespace tfmpc;

namespace {

struct Model {
    const float *F; long sF_b, sF_t;
    const float *f; long sf_b, sf_t;
    const float *C; long sC_b, sC_t;
    const float *c; long sc_b, sc_t;
    const float *Cfin; long sCfin_b;
    const float *cfin; long scfin_b;
};

int check_model(int B, int n, int m, int T, const Model &md)
{
    if (B < 0 || n <= 0 || m <= 0 || T <= 0) return TFMPC_ERR_ARG;
    if (!tvlqr_mfma_supported(n, m) && tvlqr_generic_smem_bytes(n, m) > kMaxLdsBytes) return TFMPC_ERR_UNSUPPORTED;
    if (B == 0) return TFMPC_OK;                                    // no-op: nothing is read (empty tensors may be NULL)
    if (!md.F || !md.f || !md.C || !md.c) return TFMPC_ERR_ARG;
    if (!md.Cfin != !md.cfin) return TFMPC_ERR_ARG;                 // both or neither
    for (long s : {md.sF_b, md.sF_t, md.sf_b, md.sf_t, md.sC_b, md.sC_t, md.sc_b, md.sc_t, md.sCfin_b, md.scfin_b})
        if (s < 0) return TFMPC_ERR_ARG;
    return TFMPC_OK;
}

TvLqrArgs make_args(int B, int n, int m, int T, const Model &md)
{
    TvLqrArgs a{};
    a.B = B; a.n = n; a.m = m; a.T = T;
    a.F = md.F; a.sF_b = md.sF_b; a.sF_t = md.sF_t;
    a.f = md.f; a.sf_b = md.sf_b; a.sf_t = md.sf_t;
    a.C = md.C; a.sC_b = md.sC_b; a.sC_t = md.sC_t;
    a.c = md.c; a.sc_b = md.sc_b; a.sc_t = md.sc_t;
    a.Cfin = md.Cfin; a.sCfin_b = md.sCfin_b;
    a.cfin = md.cfin; a.scfin_b = md.scfin_b;
    return a;
}

int run(const TvLqrArgs &a, bool bw, bool fw, void *stream)
{
    if (a.B == 0) return TFMPC_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (tvlqr_mfma_supported(a.n, a.m)) return tvlqr_mfma_launch(a, bw, fw, s);
    return tvlqr_generic_launch(a, bw, fw, s);
}

}  // namespace

#define TFMPC_TVLQR_MODEL_PARAMS                                                                                    \
    int B, int n, int m, int T, const float *F, long sF_b, long sF_t, const float *f, long sf_b, long sf_t,         \
        const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t, const float *Cfin, long sCfin_b, \
        const float *cfin, long scfin_b
#define TFMPC_TVLQR_MODEL Model{F, sF_b, sF_t, f, sf_b, sf_t, C, sC_b, sC_t, c, sc_b, sc_t, Cfin, sCfin_b, cfin, scfin_b}

namespace tfmpc {

int tvlqr_solve_masked_f32(TFMPC_TVLQR_MODEL_PARAMS, const float *x0, float *states, float *actions, float *costs,
                           int32_t *status, const uint32_t *mask, void *workspace, size_t workspace_bytes, void *stream)
{
    const Model md = TFMPC_TVLQR_MODEL;
    int rc = check_model(B, n, m, T, md);
    if (rc != TFMPC_OK || B == 0) return rc;
    if (!x0 || !states || !costs || !actions) return TFMPC_ERR_ARG;
    if (mask && m > 32) return TFMPC_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < tfmpc_tvlqr_workspace_bytes(B, n, m, T)) return TFMPC_ERR_WORKSPACE;
    float *w = static_cast<float *>(workspace);
    TvLqrArgs a = make_args(B, n, m, T, md);
    a.x0 = x0;
    a.K = w; a.k = w + (size_t)B * T * m * n; a.sK = (long)T * m * n; a.sk = (long)T * m;
    a.states = states; a.actions = actions; a.costs = costs; a.status = status;
    a.mask = mask;
    return run(a, true, true, stream);
}

}  // namespace tfmpc

extern "C" {

size_t tfmpc_tvlqr_workspace_bytes(int B, int n, int m, int T)
{
    if (B <= 0 || n <= 0 || m <= 0 || T <= 0) return 0;
    return (size_t)B * T * m * (n + 1) * sizeof(float);
}

const char *tfmpc_tvlqr_kernel_name(int n, int m, int T)
{
    (void)T;
    if (n <= 0 || m <= 0) return "invalid";
    if (tvlqr_mfma_supported(n, m)) return (n == 16 && m == 8) ? "tv_mfma_16x8" : "tv_mfma_16x8 (zero-padded)";
    if (tvlqr_generic_smem_bytes(n, m) > kMaxLdsBytes) return "unsupported";
    return "tv_generic_wave";
}

int tfmpc_tvlqr_backward_f32(TFMPC_TVLQR_MODEL_PARAMS, float *K, float *k, float *V, float *v, float *cst,
                             int32_t *status, void *stream)
{
    const Model md = TFMPC_TVLQR_MODEL;
    int rc = check_model(B, n, m, T, md);
    if (rc != TFMPC_OK || B == 0) return rc;
    if (B > 0 && (!K || !k)) return TFMPC_ERR_ARG;
    TvLqrArgs a = make_args(B, n, m, T, md);
    a.K = K; a.k = k; a.sK = (long)T * m * n; a.sk = (long)T * m;
    a.V = V; a.v = v; a.cst = cst; a.status = status;
    return run(a, true, false, stream);
}

int tfmpc_tvlqr_forward_f32(TFMPC_TVLQR_MODEL_PARAMS, const float *K, long strideK, const float *k, long stride_k,
                            const float *x0, float *states, float *actions, float *costs, void *stream)
{
    const Model md = TFMPC_TVLQR_MODEL;
    int rc = check_model(B, n, m, T, md);
    if (rc != TFMPC_OK || B == 0) return rc;
    if (strideK < 0 || stride_k < 0) return TFMPC_ERR_ARG;
    if (B > 0 && (!x0 || !states || !costs || !K || !k || !actions)) return TFMPC_ERR_ARG;
    TvLqrArgs a = make_args(B, n, m, T, md);
    a.x0 = x0;
    a.K = const_cast<float *>(K); a.k = const_cast<float *>(k); a.sK = strideK; a.sk = stride_k;
    a.states = states; a.actions = actions; a.costs = costs;
    return run(a, false, true, stream);
}

int tfmpc_tvlqr_solve_f32(TFMPC_TVLQR_MODEL_PARAMS, const float *x0, float *states, float *actions, float *costs,
                          float *K, float *k, float *V, float *v, float *cst, int32_t *status,
                          void *workspace, size_t workspace_bytes, void *stream)
{
    const Model md = TFMPC_TVLQR_MODEL;
    int rc = check_model(B, n, m, T, md);
    if (rc != TFMPC_OK || B == 0) return rc;
    if (B > 0 && (!x0 || !states || !costs || !actions)) return TFMPC_ERR_ARG;
    if (B > 0 && (!K || !k)) {
        // gains are not a requested output: keep them in caller-provided scratch
        if (!workspace || workspace_bytes < tfmpc_tvlqr_workspace_bytes(B, n, m, T)) return TFMPC_ERR_WORKSPACE;
        float *w = static_cast<float *>(workspace);
        if (!K) K = w;
        if (!k) k = w + (size_t)B * T * m * n;
    }
    TvLqrArgs a = make_args(B, n, m, T, md);
    a.x0 = x0;
    a.K = K; a.k = k; a.sK = (long)T * m * n; a.sk = (long)T * m;
    a.V = V; a.v = v; a.cst = cst;
    a.states = states; a.actions = actions; a.costs = costs; a.status = status;
    return run(a, true, true, stream);
}

}  // extern "C"
