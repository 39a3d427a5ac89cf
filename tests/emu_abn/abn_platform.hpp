// abn_platform.hpp (tests/emu_abn) -- SIMT-emulator implementations of the device primitives of
// ccnet_amd/csrc_abn/abn_platform.hpp, on top of the shared emulator in tests/emu/.  Test infrastructure only: the emulator
// build of the ABN kernels puts this directory FIRST on the include path; the product build never does.
#pragma once
#include "hip_emu.hpp"

#include <stdint.h>
#include <string.h>

struct uint4 {
    uint32_t x, y, z, w;
};

namespace abn {

constexpr int kWave = 64;

__device__ inline int lane_id() { return emu::lane_id(); }

// the same butterfly as the device's __shfl_xor tree, so the emulated sums round exactly like the device's
__device__ inline double wave_sum(double v) {
    for (int m = kWave / 2; m > 0; m >>= 1) {
        uint64_t mine;
        memcpy(&mine, &v, 8);
        const uint64_t *s = emu::wave_exchange(mine);
        double other;
        memcpy(&other, &s[emu::lane_id() ^ m], 8);
        v += other;
    }
    return v;
}

__device__ inline uint4 load16(const void *p) {
    if (reinterpret_cast<uintptr_t>(p) & 15) abort();          // the device load needs the alignment the caller promised
    uint4 v;
    memcpy(&v, p, 16);
    return v;
}
__device__ inline void store16(void *p, uint4 v) {
    if (reinterpret_cast<uintptr_t>(p) & 15) abort();
    memcpy(p, &v, 16);
}

}  // namespace abn

#define ABN_LAUNCH(kern, grid, block, stream, ...) emu::launch((grid), (block), [&]() { kern(__VA_ARGS__); })
