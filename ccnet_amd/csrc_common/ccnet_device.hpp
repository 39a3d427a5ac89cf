// ccnet_device.hpp -- gfx950 implementations of the device primitives that the OHEM, evaluation, Lovász and ABN kernels share
// (the wave64 lane id and butterfly sum, the LDS histogram increment, the plain launch macro).  Each library's x_platform.hpp
// includes it by its path relative to itself and pulls what it uses into its own namespace with `using`.  The CPU test-suite
// has a header of the same name under tests/emu_common/ that implements them in the SIMT emulator and that the emulator twins
// tests/emu_x/x_platform.hpp include instead; the product never sees it.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace ccnet_common {

constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }

// butterfly sum over the 64 lanes: every lane gets the same, order-fixed result
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// integer increment of an LDS counter (ds_add_u32): counts are order-independent, so the histogram stays deterministic
__device__ __forceinline__ void lds_inc(unsigned *p) { atomicAdd(p, 1u); }

}  // namespace ccnet_common

#define CCNET_LAUNCH(kern, grid, block, stream, ...) kern<<<(grid), (block), 0, (stream)>>>(__VA_ARGS__)
