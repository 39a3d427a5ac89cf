// lovasz_platform.hpp -- gfx950 implementations of the few device primitives the Lovász kernels use (wave64 ballot and
// lane rank, the butterfly sum, the LDS histogram increment, the launch macro).  The CPU test-suite has a header of the same
// name under tests/emu_lovasz/ that implements them in the SIMT emulator; the product never sees it.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace lovasz {

constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }

// 64-bit mask of the lanes of this wave whose `pred` is set (every lane of the wave must call it)
__device__ __forceinline__ uint64_t ballot(bool pred) { return (uint64_t)__ballot(pred); }

// number of set bits of `mask` below this lane (v_mbcnt_lo / v_mbcnt_hi)
__device__ __forceinline__ unsigned rank_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

__device__ __forceinline__ unsigned popc64(uint64_t m) { return (unsigned)__popcll(m); }

// butterfly sum over the 64 lanes: every lane gets the same, order-fixed result
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// integer increment of an LDS counter (ds_add_u32): counts are order-independent, so the histogram stays deterministic
__device__ __forceinline__ void lds_inc(unsigned *p) { atomicAdd(p, 1u); }

}  // namespace lovasz

#define LOVASZ_LAUNCH(kern, grid, block, stream, ...) kern<<<(grid), (block), 0, (stream)>>>(__VA_ARGS__)
