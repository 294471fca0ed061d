// batch_sum.h -- the one batch sum of the gradient kernels: "a gradient whose batch stride is 0 is summed
// over the batch in a fixed order".  The instance kernel writes per-instance records rec[b][e] (e < nE = slots * size)
// into the workspace; stage 1 adds them up over chunks of CHUNK instances, stage 2 adds up the chunks.  No atomics: the
// same call gives the same bits, and tests/batch_sum_ref.py emulates every order stated here bit for bit.
//
// Workspace in elements (floats, or doubles for the double gradients): one record array [B][slots][size] per summed
// output, each rounded up to 64 elements, in output order; then the stage-1 partial sums [chunks][nE] of the widest output
// (every output reuses them).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>

#include "../../include/tfmpc_hip.h"

namespace tfmpc {

constexpr int kSumThreads = 256;
constexpr int kSumMaxOutputs = 8;

// The stage kernels are overloads on the scalar type T of the records (float; double for the double gradients: the same
// orders, double accumulators, the workspace counted in doubles).  batch_sum_stages.h holds their one text and is included
// once per type, so the fp32 kernels keep their names and compile to the instructions they always had; the host side
// below is a template on T with float as the default.
#define TFMPC_SUM_T float
#include "batch_sum_stages.h"
#undef TFMPC_SUM_T
#define TFMPC_SUM_T double
#include "batch_sum_stages.h"
#undef TFMPC_SUM_T

enum BatchSumOrder { kSumInOrder, kSumTree };

// Where the records and partial sums of one call live in the workspace.
struct BatchSumPlan {
    int B, chunks, count;                // instances, stage-1 chunks, outputs
    unsigned summed;                     // bit q: output q is summed over the batch
    int size[kSumMaxOutputs];            // elements of output q per slot
    int slots[kSumMaxOutputs];           // T for an output with a time axis, else 1
    size_t rec_off[kSumMaxOutputs];      // in elements
    size_t partial_off, floats;          // the partial sums' offset and the workspace size, in elements (0: nothing summed)
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

// Which outputs are summed, for batch_sum_plan: bit q is set where outs[q] has batch stride sb[q] == 0 (over a batch of
// one the sum is the instance's own gradient, written in place).  With time strides st, slots[q] = steps for an output
// that has a time axis (st[q] != 0), else 1; a family without a time axis passes st = slots = nullptr.
template <class T>
inline unsigned batch_sum_select(int B, int count, T *const *outs, const long *sb, const long *st, int steps, int *slots)
{
    unsigned summed = 0;
    for (int q = 0; q < count; ++q) {
        if (slots) slots[q] = st[q] ? steps : 1;
        if (outs[q] && sb[q] == 0 && B > 1) summed |= 1u << q;
    }
    return summed;
}

// Where the instance kernel writes output q: set(q, pointer, batch stride, time stride) gets the caller's buffer and
// strides, or for a summed output its records in the workspace w, [B][slots][size] (st = nullptr: no time strides, 0).
template <class T, class Set>
inline void batch_sum_route(const BatchSumPlan &p, T *w, T *const *outs, const long *sb, const long *st, Set set)
{
    for (int q = 0; q < p.count; ++q) {
        const long size = p.size[q], t = st ? st[q] : 0;
        if (p.summed >> q & 1u) set(q, w + p.rec_off[q], (long)p.slots[q] * size, t ? size : 0);
        else set(q, outs[q], sb[q], t);
    }
}

// Enqueues stage 1 and stage 2 of every summed output: outs[q] with time stride st[q] (in-order stage 2; the tree writes
// one slot).  CHUNK is the chunk the plan was made with.  The caller returns on !p.fits before it launches anything.
template <int CHUNK, BatchSumOrder ORDER, class T = float>
inline int batch_sum_run(const BatchSumPlan &p, T *w, T *const *outs, const long *st, hipStream_t s)
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
        if constexpr (ORDER == kSumTree) {
            // one launch where the slots are dense in the output; else a launch per slot (its columns of the partial sums)
            const bool dense = p.slots[q] == 1 || st[q] == (long)p.size[q];
            const int launches = dense ? 1 : p.slots[q];
            for (int t = 0; t < launches; ++t) {
                hipLaunchKernelGGL(batch_sum_stage2_tree<kSumThreads>, dim3((unsigned)(dense ? nE : p.size[q])), dim3(kSumThreads), 0,
                                   s, w + p.partial_off + (size_t)t * p.size[q], chunks, nE, outs[q] + (size_t)t * st[q]);
                if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
            }
        } else
            hipLaunchKernelGGL(batch_sum_stage2_in_order<kSumThreads>, dim3(slices), dim3(kSumThreads), 0, s, w + p.partial_off,
                               chunks, nE, p.size[q], outs[q], st[q]);
        if (hipGetLastError() != hipSuccess) return TFMPC_ERR_LAUNCH;
    }
    return TFMPC_OK;
}

}  // namespace tfmpc
