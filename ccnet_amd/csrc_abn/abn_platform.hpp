// abn_platform.hpp -- gfx950 implementations of the few device primitives the ABN kernels use (the wave64 butterfly sum,
// 16-byte vector loads and stores, the launch macro).  The CPU test-suite has a header of the same name under tests/emu_abn/
// that implements them in the SIMT emulator; the product never sees it.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace abn {

constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }

// butterfly sum over the 64 lanes: every lane gets the same, order-fixed result
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// 16 bytes at a 16-byte aligned address (global_load_dwordx4 / global_store_dwordx4)
__device__ __forceinline__ uint4 load16(const void *p) { return *static_cast<const uint4 *>(p); }
__device__ __forceinline__ void store16(void *p, uint4 v) { *static_cast<uint4 *>(p) = v; }

}  // namespace abn

#define ABN_LAUNCH(kern, grid, block, stream, ...) kern<<<(grid), (block), 0, (stream)>>>(__VA_ARGS__)
