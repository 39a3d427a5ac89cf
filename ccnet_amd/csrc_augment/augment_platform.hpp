// augment_platform.hpp -- the device primitives the input-pipeline kernel uses: the launch macro of
// csrc_common/ccnet_device.hpp under this library's name; it has none of its own.  The CPU test-suite has a header of the same
// name under tests/emu_augment/; the product never sees it.
#pragma once
#include "../csrc_common/ccnet_device.hpp"

#define AUGMENT_LAUNCH CCNET_LAUNCH
