// lovasz_platform.hpp -- gfx950 implementations of the few device primitives the Lovász kernels use.  Its own: the wave64
// ballot and lane rank.  From csrc_common/ccnet_device.hpp: the butterfly sum, the LDS histogram increment, the launch macro.
// The CPU test-suite has a header of the same name under tests/emu_lovasz/ that implements them in the SIMT emulator; the
// product never sees it.
#pragma once
#include "../csrc_common/ccnet_device.hpp"

namespace lovasz {

using ccnet_common::kWave;
using ccnet_common::lane_id;
using ccnet_common::lds_inc;
using ccnet_common::wave_sum;

// 64-bit mask of the lanes of this wave whose `pred` is set (every lane of the wave must call it)
__device__ __forceinline__ uint64_t ballot(bool pred) { return (uint64_t)__ballot(pred); }

// number of set bits of `mask` below this lane (v_mbcnt_lo / v_mbcnt_hi)
__device__ __forceinline__ unsigned rank_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

__device__ __forceinline__ unsigned popc64(uint64_t m) { return (unsigned)__popcll(m); }

}  // namespace lovasz

#define LOVASZ_LAUNCH CCNET_LAUNCH
