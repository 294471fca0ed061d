// launch.h -- the ONE host-side launch sequence of the kernels that take their LDS as dynamic shared memory: refuse what
// no workgroup can hold, opt in above the 64 KiB a launch gets by default, launch, report.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/tfmpc_hip.h"

namespace tfmpc {

// gfx950: 160 KiB of LDS per CU, all of it addressable by one workgroup.
constexpr size_t kMaxLdsBytes = 160 * 1024;

// `smem` bytes of dynamic LDS for `kern`: above 64 KiB a kernel has to ask for them
template <class K>
bool allow_lds(K kern, size_t smem)
{
    return smem <= 64 * 1024 || hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) == hipSuccess;
}

// `blocks` workgroups of `threads` threads, `smem` bytes of dynamic LDS each
template <class K, class... Args>
int launch_with_lds(K kern, unsigned blocks, unsigned threads, size_t smem, hipStream_t stream, const Args &...args)
{
    if (smem > kMaxLdsBytes) return TFMPC_ERR_UNSUPPORTED;
    if (!allow_lds(kern, smem)) return TFMPC_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), smem, stream, args...);
    return hipGetLastError() == hipSuccess ? TFMPC_OK : TFMPC_ERR_LAUNCH;
}

}  // namespace tfmpc
