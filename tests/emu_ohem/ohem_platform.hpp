// ohem_platform.hpp (tests/emu_ohem) -- the emulator twin of ccnet_amd/csrc_ohem/ohem_platform.hpp: the same names, taken from
// the emulated primitives of tests/emu_common/ccnet_device.hpp.  Test infrastructure only: the emulator build of the OHEM
// kernels puts this directory FIRST on the include path; the product build never does.
#pragma once
#include "../emu_common/ccnet_device.hpp"

#include <math.h>

namespace ohem {

using ccnet_common::kWave;
using ccnet_common::lane_id;
using ccnet_common::lds_inc;
using ccnet_common::wave_sum;

}  // namespace ohem

#define OHEM_LAUNCH CCNET_LAUNCH
