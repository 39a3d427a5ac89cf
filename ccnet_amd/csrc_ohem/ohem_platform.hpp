// ohem_platform.hpp -- gfx950 implementations of the few device primitives the OHEM kernels use (wave64 sums, the LDS
// histogram increment, the launch macro).  The CPU test-suite has a header of the same name under tests/emu_ohem/ that
// implements them in the SIMT emulator; the product never sees it.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace ohem {

constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }

// butterfly sums over the 64 lanes: every lane gets the same, order-fixed result
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// integer increment of an LDS counter (ds_add_u32): counts are order-independent, so the histogram stays deterministic
__device__ __forceinline__ void lds_inc(unsigned *p) { atomicAdd(p, 1u); }

}  // namespace ohem

#define OHEM_LAUNCH(kern, grid, block, stream, ...) kern<<<(grid), (block), 0, (stream)>>>(__VA_ARGS__)
