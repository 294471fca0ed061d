// tvlqr_generic.hip -- shape-generic TIME-VARYING LQR (tfmpc_tvlqr_*_f32) for every shape the 16 x 8 matrix-core
// kernel does not serve (n > 16 or m > 8), up to one wave's LDS: one wavefront per instance, fp32.
//
// The fp32 instantiation of tvlqr_wave.h's body: products on the f32 matrix cores (wave_ops.h), every LDS buffer its own.
// The fallback, not a performance target.
#include <hip/hip_runtime.h>

#include "tvlqr_wave.h"

namespace tfmpc {

namespace {

struct TvF32 : WaveF32 {
    static constexpr bool kFold = false;
    static __device__ __forceinline__ bool valid(float x) { return x == x; }           // not NaN (infinity passes)
};

static_assert(tv_smem_elems<false>(20, 10) == 4691, "the LDS size sets which shapes are supported");

template <bool BACKWARD, bool FORWARD>
__global__ __launch_bounds__(kWave) void tvlqr_generic_kernel(TvLqrArgs a)
{
    extern __shared__ float smem[];
    tvlqr_wave_body<TvF32, BACKWARD, FORWARD, false>(a, smem);
}

// The fused solve on a masked model (tvlqr_solve_masked_f32).
__global__ __launch_bounds__(kWave) void tvlqr_generic_masked_sweep(TvLqrArgs a)
{
    extern __shared__ float smem[];
    tvlqr_wave_body<TvF32, true, true, true>(a, smem);
}

}  // namespace

size_t tvlqr_generic_smem_bytes(int n, int m) { return tv_smem_elems<false>(n, m) * sizeof(float); }

int tvlqr_generic_launch(const TvLqrArgs &a, bool backward, bool forward, hipStream_t stream)
{
    const size_t smem = tvlqr_generic_smem_bytes(a.n, a.m);
    if (a.mask) {
        if (!(backward && forward) || a.V || a.v || a.cst) return TFMPC_ERR_ARG;
        return tv_wave_launch(tvlqr_generic_masked_sweep, a, smem, stream);
    }
    if (backward && forward) return tv_wave_launch(tvlqr_generic_kernel<true, true>, a, smem, stream);
    if (backward) return tv_wave_launch(tvlqr_generic_kernel<true, false>, a, smem, stream);
    return tv_wave_launch(tvlqr_generic_kernel<false, true>, a, smem, stream);
}

}  // namespace tfmpc
