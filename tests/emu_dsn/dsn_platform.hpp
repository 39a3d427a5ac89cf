// dsn_platform.hpp (tests/emu_dsn) -- the emulator twin of ccnet_amd/csrc_dsn/dsn_platform.hpp: the same names, taken from
// the emulated primitives of tests/emu_common/ccnet_device.hpp.  Test infrastructure only: the emulator build of the DSN
// kernels puts this directory FIRST on the include path; the product build never does.
#pragma once
#include "../emu_common/ccnet_device.hpp"

#include <math.h>

namespace dsn {

using ccnet_common::kWave;
using ccnet_common::lane_id;
using ccnet_common::wave_sum;

}  // namespace dsn

#define DSN_LAUNCH CCNET_LAUNCH
