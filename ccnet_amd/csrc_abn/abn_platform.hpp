// abn_platform.hpp -- gfx950 implementations of the few device primitives the ABN kernels use.  Its own: 16-byte vector loads
// and stores.  From csrc_common/ccnet_device.hpp: the wave64 butterfly sum and the launch macro.  The CPU test-suite has a
// header of the same name under tests/emu_abn/ that implements them in the SIMT emulator; the product never sees it.
#pragma once
#include "../csrc_common/ccnet_device.hpp"

namespace abn {

using ccnet_common::kWave;
using ccnet_common::lane_id;
using ccnet_common::wave_sum;

// 16 bytes at a 16-byte aligned address (global_load_dwordx4 / global_store_dwordx4)
__device__ __forceinline__ uint4 load16(const void *p) { return *static_cast<const uint4 *>(p); }
__device__ __forceinline__ void store16(void *p, uint4 v) { *static_cast<uint4 *>(p) = v; }

}  // namespace abn

#define ABN_LAUNCH CCNET_LAUNCH
