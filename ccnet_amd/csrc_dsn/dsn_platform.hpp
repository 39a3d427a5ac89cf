// dsn_platform.hpp -- the device primitives the DSN cross-entropy kernels use (wave64 sums, the launch macro): all of them the
// shared ones of csrc_common/ccnet_device.hpp under this library's names; it has none of its own.  The CPU test-suite has a
// header of the same name under tests/emu_dsn/; the product never sees it.
#pragma once
#include "../csrc_common/ccnet_device.hpp"

namespace dsn {

using ccnet_common::kWave;
using ccnet_common::lane_id;
using ccnet_common::wave_sum;

}  // namespace dsn

#define DSN_LAUNCH CCNET_LAUNCH
