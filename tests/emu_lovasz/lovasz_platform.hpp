// lovasz_platform.hpp (tests/emu_lovasz) -- SIMT-emulator implementations of the device primitives of
// ccnet_amd/csrc_lovasz/lovasz_platform.hpp, on top of the shared emulator in tests/emu/ and the shared primitives of
// tests/emu_common/.  Test infrastructure only: the emulator build of the Lovász kernels puts this directory FIRST on the
// include path; the product build never does.
#pragma once
#include "../emu_common/ccnet_device.hpp"

namespace lovasz {

using ccnet_common::kWave;
using ccnet_common::lane_id;
using ccnet_common::lds_inc;
using ccnet_common::wave_sum;

__device__ inline uint64_t ballot(bool pred) {
    const uint64_t *s = emu::wave_exchange(pred ? 1u : 0u);
    uint64_t m = 0;
    for (int l = 0; l < kWave; ++l)
        if (s[l]) m |= uint64_t(1) << l;
    return m;
}

__device__ inline unsigned rank_below(uint64_t mask) {
    const int l = emu::lane_id();
    return (unsigned)__builtin_popcountll(l ? mask & ((uint64_t(1) << l) - 1) : 0);
}

__device__ inline unsigned popc64(uint64_t m) { return (unsigned)__builtin_popcountll(m); }

}  // namespace lovasz

#define LOVASZ_LAUNCH CCNET_LAUNCH
