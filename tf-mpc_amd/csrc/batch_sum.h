// batch_sum.h -- the one batch sum of the gradient kernels: "a gradient whose batch stride is 0 is summed
// over the batch in a fixed order".  The instance kernel writes per-instance records rec[b][e] (e < nE = slots * size)
// into the workspace; stage 1 adds them up over chunks of CHUNK instances, stage 2 adds up the chunks.  No atomics: the
// same call gives the same bits, and tests/batch_sum_ref.py emulates every order stated here bit for bit.
//
// Workspace in floats: one record array [B][slots][size] per summed output, each rounded up to 64 floats, in output
// order; then the stage-1 partial sums [chunks][nE] of the widest output (every output reuses them).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>

#include "../../include/tfmpc_hip.h"

namespace tfmpc {

constexpr int kSumThreads = 256;
constexpr int kSumMaxOutputs = 8;

// partial[chunk][e] = sum of rec[b][e] over the chunk's instances b0 = chunk * CHUNK <= b < min(B, b0 + CHUNK): four
// interleaved running sums from 0 (instance b0 + 4 i + q into s[q]; the instances left after the last full group of four
// into s[0], s[1], s[2]), then (s[0] + s[1]) + (s[2] + s[3]).  One grid axis: block = chunk * slices + element slice.
template <int CHUNK>
__global__ void __launch_bounds__(kSumThreads) batch_sum_stage1(const float *rec, int B, size_t nE, float *partial)
{
    const unsigned slices = (unsigned)((nE + kSumThreads - 1) / kSumThreads);
    const int chunk = blockIdx.x / slices;
    const size_t e = (size_t)(blockIdx.x - chunk * slices) * kSumThreads + threadIdx.x;
    if (e >= nE) return;
    const int b0 = chunk * CHUNK, b1 = min(B, b0 + CHUNK);
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int bb = b0;
    for (; bb + 4 <= b1; bb += 4)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += rec[(size_t)(bb + q) * nE + e];
    for (int q = 0; bb < b1; ++bb, ++q) s[q] += rec[(size_t)bb * nE + e];
    partial[(size_t)chunk * nE + e] = (s[0] + s[1]) + (s[2] + s[3]);
}

// Both stage-2 kernels are templates so that a translation unit holds only the one it launches.
//
// In-order stage 2: out[(e / size) * st + e % size] = 0 + partial[0][e] + partial[1][e] + ... + partial[chunks - 1][e],
// one chunk after the other (slot e / size of an output with time stride st).
template <int THREADS>
__global__ void __launch_bounds__(THREADS) batch_sum_stage2_in_order(const float *partial, int chunks, size_t nE, int size, float *out,
                                                                     long st)
{
    const size_t e = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= nE) return;
    float s = 0.0f;
    for (int k = 0; k < chunks; ++k) s += partial[(size_t)k * nE + e];
    out[(e / size) * (size_t)st + e % size] = s;
}

// Tree stage 2: one block of THREADS = 256 per element e.  Thread t adds, from 0, partial[t][e], partial[t + 256][e], ...
// in that order; then the halving tree over the 256 sub-sums in LDS, t[i] += t[i + w] for i < w, w = 128, 64, ..., 1;
// out[e] = t[0].
template <int THREADS>
__global__ void __launch_bounds__(THREADS) batch_sum_stage2_tree(const float *partial, int chunks, size_t nE, float *out)
{
    __shared__ float t[THREADS];
    const int e = blockIdx.x, tid = threadIdx.x;
    float s = 0.0f;
    for (int k = tid; k < chunks; k += THREADS) s += partial[(size_t)k * nE + e];
    t[tid] = s;
    __syncthreads();
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) t[tid] += t[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[e] = t[0];
}

enum BatchSumOrder { kSumInOrder, kSumTree };

// Where the records and partial sums of one call live in the workspace.
struct BatchSumPlan {
    int B, chunks, count;                // instances, stage-1 chunks, outputs
    unsigned summed;                     // bit q: output q is summed over the batch
    int size[kSumMaxOutputs];            // elements of output q per slot
    int slots[kSumMaxOutputs];           // T for an output with a time axis, else 1
    size_t rec_off[kSumMaxOutputs];      // in floats
    size_t partial_off, floats;          // the partial sums' offset and the workspace size, in floats (0: nothing summed)
    bool fits;                           // every stage-1 grid fits one grid axis
};

inline size_t batch_sum_up64(size_t x) { return (x + 63) / 64 * 64; }

inline BatchSumPlan batch_sum_plan(int B, int chunk, int count, const int *size, const int *slots, unsigned summed)
{
    BatchSumPlan p{};
    const size_t chunks = ((size_t)B + chunk - 1) / chunk;
    p.B = B; p.chunks = (int)chunks; p.count = count; p.summed = summed;
    p.fits = true;
    size_t o = 0, widest = 0;
    for (int q = 0; q < count; ++q) {
        p.size[q] = size[q];
        p.slots[q] = slots[q];
        if (!(summed >> q & 1u)) continue;
        const size_t nE = (size_t)slots[q] * size[q];
        p.rec_off[q] = o;
        o += batch_sum_up64((size_t)B * nE);
        widest = widest > nE ? widest : nE;
        if (chunks * ((nE + kSumThreads - 1) / kSumThreads) > (size_t)INT_MAX) p.fits = false;
    }
    p.partial_off = o;
    p.floats = summed ? o + batch_sum_up64(chunks * widest) : 0;
    return p;
}

// Enqueues stage 1 and stage 2 of every summed output: outs[q] with time stride st[q] (in-order stage 2; the tree writes
// one slot).  CHUNK is the chunk the plan was made with.  The caller returns on !p.fits before it launches anything.
template <int CHUNK, BatchSumOrder ORDER>
inline int batch_sum_run(const BatchSumPlan &p, float *w, float *const *outs, const long *st, hipStream_t s)
{
    if (!p.fits) return TFMPC_ERR_UNSUPPORTED;
    const int chunks = p.chunks;
    for (int q = 0; q < p.count; ++q) {
        if (!(p.summed >> q & 1u)) continue;
        const size_t nE = (size_t)p.slots[q] * p.size[q];
        const unsigned slices = (unsigned)((nE + kSumThreads - 1) / kSumThreads);
        hipLaunchKernelGGL(batch_sum_stage1<CHUNK>, dim3(chunks * slices), dim3(kSumThreads), 0, s, w + p.rec_off[q], p.B, nE,
                           w + p.partial_off);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
        if constexpr (ORDER == kSumTree)
            hipLaunchKernelGGL(batch_sum_stage2_tree<kSumThreads>, dim3((unsigned)nE), dim3(kSumThreads), 0, s, w + p.partial_off,
                               chunks, nE, outs[q]);
        else
            hipLaunchKernelGGL(batch_sum_stage2_in_order<kSumThreads>, dim3(slices), dim3(kSumThreads), 0, s, w + p.partial_off,
                               chunks, nE, p.size[q], outs[q], st[q]);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    return TFMPC_OK;
}

}  // namespace tfmpc
