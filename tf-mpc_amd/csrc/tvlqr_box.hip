// tvlqr_box.hip -- control-limited TIME-VARYING LQR, the forward solve (tfmpc_tvlqr_box_solve_f32): the
// fp32 instantiation of tvlqr_box_body.h, which holds the algorithm (policy and entry point: tvlqr_box_wave.h).  One wavefront per instance, the LDS layout
// and per-step model copy of tvlqr_wave.h's fp32 policy, products on the f32 matrix cores.  The double instantiation is
// in tvlqr_box_f64.hip: this file compiles to the ONE fp32 kernel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tvlqr_box_wave.h"

namespace tfmpc {

namespace {

struct TvBoxF32 : WaveF32 {
    static constexpr float kArmijo = 1e-4f, kTrustRatio = 1e-6f, kDefaultTol = 4e-6f;
};

__global__ __launch_bounds__(kWave) void tvlqr_box_solve_kernel(TvBoxArgsT<float> p)
{
    extern __shared__ float smem[];
    using P = TvBoxF32;
#include "tvlqr_box_body.h"
}

bool box_supported(int n, int m) { return m <= 32 && tv_smem_elems<false>(n, m) * sizeof(float) <= kMaxLdsBytes; }

}  // namespace

}  // namespace tfmpc

using namespace tfmpc;

extern "C" {

size_t tfmpc_tvlqr_box_solve_workspace_bytes(int B, int n, int m, int T)
{
    if (B <= 0 || n <= 0 || m <= 0 || T <= 0) return 0;
    return tv_box_workspace_elems(B, n, m, T) * sizeof(float);
}

const char *tfmpc_tvlqr_box_solve_kernel_name(int n, int m, int T)
{
    (void)T;
    if (n <= 0 || m <= 0) return "invalid";
    return box_supported(n, m) ? "tv_box_wave" : "unsupported";
}

int tfmpc_tvlqr_box_solve_f32(int B, int n, int m, int T, const float *F, long sF_b, long sF_t, const float *f, long sf_b,
                              long sf_t, const float *C, long sC_b, long sC_t, const float *c, long sc_b, long sc_t,
                              const float *Cfin, long sCfin_b, const float *cfin, long scfin_b, const float *low, long slow_b,
                              long slow_t, const float *high, long shigh_b, long shigh_t, const float *x0, const float *u_init,
                              long su_b, int max_iter, float tol, float *states, float *actions, float *costs,
                              int32_t *iterations, int32_t *status, int32_t *reason, uint32_t *clamp_mask, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    return tv_box_solve<float>(tvlqr_box_solve_kernel, n > 0 && m > 0 && box_supported(n, m), B, n, m, T, F, sF_b, sF_t, f, sf_b,
                               sf_t, C, sC_b, sC_t, c, sc_b, sc_t, Cfin, sCfin_b, cfin, scfin_b, low, slow_b, slow_t, high, shigh_b,
                               shigh_t, x0, u_init, su_b, max_iter, tol, states, actions, costs, iterations, status, reason,
                               clamp_mask, workspace, workspace_bytes, stream);
}

}  // extern "C"
