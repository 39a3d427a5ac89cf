// sgdmp_platform.hpp (tests/emu_sgdmp) -- the emulator twin of ccnet_amd/csrc_sgdmp/sgdmp_platform.hpp: the same names, the
// launch taken from the emulated one of tests/emu_common/ccnet_device.hpp, a 16-byte vector of its own, since
// tests/emu/hip_emu.hpp has no float4, and plain pointers.  Test infrastructure only: the emulator build of the mixed-precision
// optimiser kernels puts this directory FIRST on the include path; the product build never does.
#pragma once
#include "../emu_common/ccnet_device.hpp"

#define SGDMP_LAUNCH CCNET_LAUNCH

namespace sgdmp {

struct alignas(16) vec4 {
    float x, y, z, w;
};

template <class T>
using global_ptr = T *;

}  // namespace sgdmp
