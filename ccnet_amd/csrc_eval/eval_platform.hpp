// eval_platform.hpp -- gfx950 implementations of the few device primitives the evaluation kernel uses (the LDS and global
// integer adds, the dynamic LDS array, the launch macro).  The CPU test-suite has a header of the same name under
// tests/emu_eval/ that implements them in the SIMT emulator; the product never sees it.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace segeval {

// integer add to an LDS word (ds_add_u32): counts are order-independent, so the histogram stays deterministic
__device__ __forceinline__ void lds_add(unsigned *p, unsigned v) { atomicAdd(p, v); }

// integer add to a confusion cell in global memory (global_atomic_add_x2, device scope)
__device__ __forceinline__ void global_add(int64_t *p, unsigned v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}

// lets `kern` launch with `bytes` of dynamic LDS (above 64 KiB the runtime asks for the attribute)
inline int allow_dynamic_lds(const void *kern, int bytes) {
    return hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess ? 0 : -1;
}

}  // namespace segeval

#define EVAL_DYNAMIC_LDS(name) extern __shared__ unsigned name[]
#define EVAL_LAUNCH(kern, grid, block, lds_bytes, stream, ...) kern<<<(grid), (block), (lds_bytes), (stream)>>>(__VA_ARGS__)
