// lovasz_platform.hpp (tests/emu_lovasz) -- SIMT-emulator implementations of the device primitives of
// ccnet_amd/csrc_lovasz/lovasz_platform.hpp, on top of the shared emulator in tests/emu/.  Test infrastructure only: the
// emulator build of the Lovász kernels puts this directory FIRST on the include path; the product build never does.
#pragma once
#include "hip_emu.hpp"

#include <stdint.h>
#include <string.h>

namespace lovasz {

constexpr int kWave = 64;

__device__ inline int lane_id() { return emu::lane_id(); }

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

// fibers switch only at barriers and collectives, so a plain increment is atomic here
__device__ inline void lds_inc(unsigned *p) { *p += 1u; }

}  // namespace lovasz

#define LOVASZ_LAUNCH(kern, grid, block, stream, ...) emu::launch((grid), (block), [&]() { kern(__VA_ARGS__); })
