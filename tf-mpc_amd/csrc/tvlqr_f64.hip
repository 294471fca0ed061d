// tvlqr_f64.hip -- DOUBLE-PRECISION time-varying LQR (tfmpc_tvlqr_*_f64): one wavefront per instance,
// n <= 32 and m <= 32.
//
// The double instantiation of tvlqr_wave.h's body: products on v_mfma_f64_16x16x4_f64 (wave_ops_f64.h), the folded LDS
// layout.  Also the expand kernels of the time-parallel solve and of the periodic steady state (3.25):
// the same body on one segment of the horizon / of the period.  The entry points are in tvlqr_dispatch.hip.
#include <hip/hip_runtime.h>

#include "tvlqr_wave.h"

namespace tfmpc {

namespace {

constexpr int kTvF64MaxDim = 32;

// MAXD: the compile-time bound on n and m (16 or 32), i.e. on the k-steps of every matrix product.
template <int MAXD>
struct TvF64 : WaveF64<MAXD> {
    static constexpr bool kFold = true;
    static __device__ __forceinline__ bool valid(double x) { return finite(x); }       // neither NaN nor infinity
};

// 15.4 KiB at n = 16, m = 8 (ten waves per CU), 84.75 KiB at n = m = 32 (one)
static_assert(tv_smem_elems<true>(16, 8) == 1968 && tv_smem_elems<true>(32, 32) == 10848,
              "the LDS size sets which shapes are supported");

template <int MAXD, bool BACKWARD, bool FORWARD>
__global__ __launch_bounds__(kWave) void tvlqr_f64_kernel(TvLqrArgsT<double> a)
{
    extern __shared__ double smem_f64[];
    tvlqr_wave_body<TvF64<MAXD>, BACKWARD, FORWARD, false>(a, smem_f64);
}

template <int MAXD>
int launch_for(const TvLqrArgsT<double> &a, bool backward, bool forward, hipStream_t stream)
{
    const size_t smem = tv_smem_elems<true>(a.n, a.m) * sizeof(double);
    if (backward && forward) return tv_wave_launch(tvlqr_f64_kernel<MAXD, true, true>, a, smem, stream);
    if (backward) return tv_wave_launch(tvlqr_f64_kernel<MAXD, true, false>, a, smem, stream);
    return tv_wave_launch(tvlqr_f64_kernel<MAXD, false, true>, a, smem, stream);
}

// The expand phase of the time-parallel solve: the same body on segment i of instance b, between the
// stitch's boundary state and the value function behind the segment.
template <int MAXD>
__global__ __launch_bounds__(kWave) void tvlqr_expand_f64_kernel(TvLqrArgsT<double> a, TvTimeParallel tp)
{
    extern __shared__ double smem_f64[];
    const size_t w = blockIdx.x;
    const int n = a.n;
    TvSegment<double> seg;
    seg.b = (int)(blockIdx.x / (unsigned)tp.segments);
    const int i = (int)blockIdx.x - seg.b * tp.segments;
    seg.t0 = i * tp.len;
    seg.len = a.T - seg.t0 < tp.len ? a.T - seg.t0 : tp.len;
    seg.last = i == tp.segments - 1;
    seg.Vend = tp.Vend + w * n * n;
    seg.vend = tp.vend + w * n;
    seg.xstart = tp.xstart + w * n;
    seg.status = tp.st_expand + w;
    tvlqr_wave_body<TvF64<MAXD>, true, true, false>(a, smem_f64, seg);
}

template <int MAXD>
int expand_for(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, hipStream_t stream)
{
    const size_t smem = tv_smem_elems<true>(a.n, a.m) * sizeof(double);
    return launch_with_lds(tvlqr_expand_f64_kernel<MAXD>, (unsigned)a.B * tp.segments, kWave, smem, stream, a, tp);
}

// The expand phase of the periodic steady state: the body's backward sweep alone on segment i of the
// period, from the value function the periodic stitch left behind the segment; no rollout, no final cost.  The waves
// of an instance that condense or stitch flagged do not run (the finish kernel fills its outputs).
template <int MAXD>
__global__ __launch_bounds__(kWave) void tvlqr_periodic_expand_f64_kernel(TvLqrArgsT<double> a, TvTimeParallel tp)
{
    extern __shared__ double smem_f64[];
    const size_t w = blockIdx.x;
    const int n = a.n, lane = lane_id();
    TvSegment<double> seg;
    seg.b = (int)(blockIdx.x / (unsigned)tp.segments);
    const int i = (int)blockIdx.x - seg.b * tp.segments;
    int flagged = lane == 0 ? tp.st_stitch[seg.b] : 0;
    for (int s = lane; s < tp.segments; s += kWave) flagged |= tp.st_condense[(size_t)seg.b * tp.segments + s];
    if (__ballot(flagged != 0)) {
        if (lane == 0) tp.st_expand[w] = 0;
        return;
    }
    seg.t0 = i * tp.len;
    seg.len = a.T - seg.t0 < tp.len ? a.T - seg.t0 : tp.len;
    seg.last = false;
    seg.Vend = tp.Vend + w * n * n;
    seg.vend = tp.vend + w * n;
    seg.xstart = nullptr;
    seg.status = tp.st_expand + w;
    tvlqr_wave_body<TvF64<MAXD>, true, false, false, TvSegment<double>>(a, smem_f64, seg);
}

template <int MAXD>
int periodic_expand_for(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, hipStream_t stream)
{
    const size_t smem = tv_smem_elems<true>(a.n, a.m) * sizeof(double);
    return launch_with_lds(tvlqr_periodic_expand_f64_kernel<MAXD>, (unsigned)a.B * tp.segments, kWave, smem, stream, a, tp);
}

// The masked sweep (tvlqr_solve_masked_f64): the body with the held controls taken out of each step's
// model; FORWARD = false is the backward sweep alone, for a caller that wants the value function only.
template <int MAXD, bool FORWARD>
__global__ __launch_bounds__(kWave) void tvlqr_masked_f64_sweep(TvLqrArgsT<double> a)
{
    extern __shared__ double smem_f64[];
    tvlqr_wave_body<TvF64<MAXD>, true, FORWARD, true>(a, smem_f64);
}

template <int MAXD>
int masked_for(const TvLqrArgsT<double> &a, bool forward, hipStream_t stream)
{
    const size_t smem = tv_smem_elems<true>(a.n, a.m) * sizeof(double);
    if (forward) return tv_wave_launch(tvlqr_masked_f64_sweep<MAXD, true>, a, smem, stream);
    return tv_wave_launch(tvlqr_masked_f64_sweep<MAXD, false>, a, smem, stream);
}

}  // namespace

bool tvlqr_f64_supported(int n, int m) { return n <= kTvF64MaxDim && m <= kTvF64MaxDim; }

const char *tvlqr_f64_kernel_name(int n, int m) { return wave16(n, m) ? "tv_f64_wave16" : "tv_f64_wave32"; }

int tvlqr_f64_launch(const TvLqrArgsT<double> &a, bool backward, bool forward, hipStream_t stream)
{
    return wave16(a.n, a.m) ? launch_for<16>(a, backward, forward, stream) : launch_for<32>(a, backward, forward, stream);
}

const char *tvlqr_f64_masked_kernel_name(int n, int m) { return wave16(n, m) ? "tv_masked_f64_wave16" : "tv_masked_f64_wave32"; }

int tvlqr_f64_masked_launch(const TvLqrArgsT<double> &a, bool forward, hipStream_t stream)
{
    return wave16(a.n, a.m) ? masked_for<16>(a, forward, stream) : masked_for<32>(a, forward, stream);
}

int tvlqr_f64_expand_launch(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, hipStream_t stream)
{
    return wave16(a.n, a.m) ? expand_for<16>(a, tp, stream) : expand_for<32>(a, tp, stream);
}

int tvlqr_f64_periodic_expand_launch(const TvLqrArgsT<double> &a, const TvTimeParallel &tp, hipStream_t stream)
{
    return wave16(a.n, a.m) ? periodic_expand_for<16>(a, tp, stream) : periodic_expand_for<32>(a, tp, stream);
}

}  // namespace tfmpc
