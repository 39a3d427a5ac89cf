// augment_platform.hpp (tests/emu_augment) -- the emulator twin of ccnet_amd/csrc_augment/augment_platform.hpp: the same
// name, taken from the emulated launch of tests/emu_common/ccnet_device.hpp.  Test infrastructure only: the emulator build of
// the input-pipeline kernel puts this directory FIRST on the include path; the product build never does.
#pragma once
#include "../emu_common/ccnet_device.hpp"

#define AUGMENT_LAUNCH CCNET_LAUNCH
