// batch_sum_stages.h -- the stage kernels of batch_sum.h for ONE scalar type, TFMPC_SUM_T.  batch_sum.h includes this
// file once per type (float, double) inside namespace tfmpc, which is why it has no include guard and opens no namespace:
// the kernels are overloads on the pointer type, and each type's kernels are this text compiled as written.
#ifndef TFMPC_SUM_T
#error "batch_sum_stages.h is included by batch_sum.h with TFMPC_SUM_T defined"
#endif

// partial[chunk][e] = sum of rec[b][e] over the chunk's instances b0 = chunk * CHUNK <= b < min(B, b0 + CHUNK): four
// interleaved running sums from 0 (instance b0 + 4 i + q into s[q]; the instances left after the last full group of four
// into s[0], s[1], s[2]), then (s[0] + s[1]) + (s[2] + s[3]).  One grid axis: block = chunk * slices + element slice.
template <int CHUNK>
__global__ void __launch_bounds__(kSumThreads) batch_sum_stage1(const TFMPC_SUM_T *rec, int B, size_t nE, TFMPC_SUM_T *partial)
{
    const unsigned slices = (unsigned)((nE + kSumThreads - 1) / kSumThreads);
    const int chunk = blockIdx.x / slices;
    const size_t e = (size_t)(blockIdx.x - chunk * slices) * kSumThreads + threadIdx.x;
    if (e >= nE) return;
    const int b0 = chunk * CHUNK, b1 = min(B, b0 + CHUNK);
    TFMPC_SUM_T s[4] = {0, 0, 0, 0};
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
__global__ void __launch_bounds__(THREADS) batch_sum_stage2_in_order(const TFMPC_SUM_T *partial, int chunks, size_t nE, int size,
                                                                     TFMPC_SUM_T *out, long st)
{
    const size_t e = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= nE) return;
    TFMPC_SUM_T s = 0;
    for (int k = 0; k < chunks; ++k) s += partial[(size_t)k * nE + e];
    out[(e / size) * (size_t)st + e % size] = s;
}

// Tree stage 2: one block of THREADS = 256 per element e.  Thread t adds, from 0, partial[t][e], partial[t + 256][e], ...
// in that order; then the halving tree over the 256 sub-sums in LDS, t[i] += t[i + w] for i < w, w = 128, 64, ..., 1;
// out[e] = t[0].
template <int THREADS>
__global__ void __launch_bounds__(THREADS) batch_sum_stage2_tree(const TFMPC_SUM_T *partial, int chunks, size_t nE, TFMPC_SUM_T *out)
{
    __shared__ TFMPC_SUM_T t[THREADS];
    const int e = blockIdx.x, tid = threadIdx.x;
    TFMPC_SUM_T s = 0;
    for (int k = tid; k < chunks; k += THREADS) s += partial[(size_t)k * nE + e];
    t[tid] = s;
    __syncthreads();
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) t[tid] += t[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[e] = t[0];
}
