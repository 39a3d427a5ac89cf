// ccnet_device.hpp (tests/emu_common) -- SIMT-emulator implementations of the device primitives of
// ccnet_amd/csrc_common/ccnet_device.hpp, on top of the shared emulator in tests/emu/.  Test infrastructure only: the emulator
// twins tests/emu_x/x_platform.hpp include it by relative path where the product's x_platform.hpp include the device one; the
// product build never sees it.
#pragma once
#include "hip_emu.hpp"

#include <stdint.h>
#include <string.h>

namespace ccnet_common {

constexpr int kWave = 64;

__device__ inline int lane_id() { return emu::lane_id(); }

// the same butterfly as the device's __shfl_xor tree, so the emulated sums round exactly like the device's
template <class T>
__device__ inline T wave_sum(T v) {
    static_assert(sizeof(T) <= 8, "one 64-bit payload per lane");
    for (int m = kWave / 2; m > 0; m >>= 1) {
        uint64_t mine = 0;
        memcpy(&mine, &v, sizeof(T));
        const uint64_t *s = emu::wave_exchange(mine);
        T other;
        memcpy(&other, &s[emu::lane_id() ^ m], sizeof(T));
        v += other;
    }
    return v;
}

// fibers switch only at barriers and collectives, so a plain increment is atomic here
__device__ inline void lds_inc(unsigned *p) { *p += 1u; }

}  // namespace ccnet_common

#define CCNET_LAUNCH(kern, grid, block, stream, ...) emu::launch((grid), (block), [&]() { kern(__VA_ARGS__); })
