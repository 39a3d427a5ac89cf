// ohem_platform.hpp -- the device primitives the OHEM kernels use (wave64 sums, the LDS histogram increment, the launch macro):
// all of them the shared ones of csrc_common/ccnet_device.hpp under this library's names.  The CPU test-suite has a header of
// the same name under tests/emu_ohem/; the product never sees it.
#pragma once
#include "../csrc_common/ccnet_device.hpp"

namespace ohem {

using ccnet_common::kWave;
using ccnet_common::lane_id;
using ccnet_common::lds_inc;
using ccnet_common::wave_sum;

}  // namespace ohem

#define OHEM_LAUNCH CCNET_LAUNCH
