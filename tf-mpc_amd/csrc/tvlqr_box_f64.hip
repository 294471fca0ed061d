// tvlqr_box_f64.hip -- DOUBLE-PRECISION control-limited time-varying LQR, the forward solve (tfmpc_tvlqr_box_solve_f64,
// DESIGN.md 3.18): one wavefront per instance, n <= 32 and m <= 32.
//
// The double instantiation of tvlqr_box_body.h (policy and entry point: tvlqr_box_wave.h): products on v_mfma_f64_16x16x4_f64 (wave_ops_f64.h), the
// elimination on wave_gauss_jordan<false> in double, the unfolded LDS layout.
#include <hip/hip_runtime.h>

#include "tvlqr_box_wave.h"

namespace tfmpc {

namespace {

constexpr int kTvBoxF64MaxDim = 32;

// MAXD: the compile-time bound on n and m (16 or 32), i.e. on the k-steps of every matrix product.
template <int MAXD>
struct TvBoxF64 : WaveF64<MAXD> {
    static constexpr double kArmijo = 1e-4, kTrustRatio = 1e-6, kDefaultTol = 1e-12;
};

// 23.9 KiB at n = 16, m = 8 (six waves per CU), 142.3 KiB at n = m = 32 (one)
static_assert(tv_smem_elems<false>(16, 8) == 3065 && tv_smem_elems<false>(32, 32) == 18209,
              "the LDS size sets the resident waves");
static_assert(tv_smem_elems<false>(kTvBoxF64MaxDim, kTvBoxF64MaxDim) * sizeof(double) <= kMaxLdsBytes,
              "every supported shape fits one wave's LDS");

template <int MAXD>
__global__ __launch_bounds__(kWave) void tvlqr_box_solve_f64_kernel(TvBoxArgsT<double> p)
{
    extern __shared__ double smem[];
    using P = TvBoxF64<MAXD>;
#include "tvlqr_box_body.h"
}

bool box_f64_supported(int n, int m) { return n <= kTvBoxF64MaxDim && m <= kTvBoxF64MaxDim; }

}  // namespace

}  // namespace tfmpc

using namespace tfmpc;

extern "C" {

size_t tfmpc_tvlqr_box_solve_workspace_bytes_f64(int B, int n, int m, int T)
{
    if (B <= 0 || n <= 0 || m <= 0 || T <= 0) return 0;
    return tv_box_workspace_elems(B, n, m, T) * sizeof(double);
}

const char *tfmpc_tvlqr_box_solve_kernel_name_f64(int n, int m, int T)
{
    (void)T;
    if (n <= 0 || m <= 0) return "invalid";
    if (!box_f64_supported(n, m)) return "unsupported";
    return wave16(n, m) ? "tv_box_f64_wave16" : "tv_box_f64_wave32";
}

int tfmpc_tvlqr_box_solve_f64(int B, int n, int m, int T, const double *F, long sF_b, long sF_t, const double *f, long sf_b,
                              long sf_t, const double *C, long sC_b, long sC_t, const double *c, long sc_b, long sc_t,
                              const double *Cfin, long sCfin_b, const double *cfin, long scfin_b, const double *low,
                              long slow_b, long slow_t, const double *high, long shigh_b, long shigh_t, const double *x0,
                              const double *u_init, long su_b, int max_iter, double tol, double *states, double *actions,
                              double *costs, int32_t *iterations, int32_t *status, int32_t *reason, uint32_t *clamp_mask,
                              void *workspace, size_t workspace_bytes, void *stream)
{
    const bool small = n > 0 && m > 0 && wave16(n, m);
    return tv_box_solve<double>(small ? tvlqr_box_solve_f64_kernel<16> : tvlqr_box_solve_f64_kernel<32>,
                                n > 0 && m > 0 && box_f64_supported(n, m), B, n, m, T, F, sF_b, sF_t, f, sf_b, sf_t, C, sC_b,
                                sC_t, c, sc_b, sc_t, Cfin, sCfin_b, cfin, scfin_b, low, slow_b, slow_t, high, shigh_b, shigh_t,
                                x0, u_init, su_b, max_iter, tol, states, actions, costs, iterations, status, reason,
                                clamp_mask, workspace, workspace_bytes, stream);
}

}  // extern "C"
