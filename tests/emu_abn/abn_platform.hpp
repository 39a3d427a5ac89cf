// abn_platform.hpp (tests/emu_abn) -- SIMT-emulator implementations of the device primitives of
// ccnet_amd/csrc_abn/abn_platform.hpp, on top of the shared emulator in tests/emu/ and the shared primitives of
// tests/emu_common/.  Test infrastructure only: the emulator build of the ABN kernels puts this directory FIRST on the include
// path; the product build never does.
#pragma once
#include "../emu_common/ccnet_device.hpp"

struct uint4 {
    uint32_t x, y, z, w;
};

namespace abn {

using ccnet_common::kWave;
using ccnet_common::lane_id;
using ccnet_common::wave_sum;

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

#define ABN_LAUNCH CCNET_LAUNCH
