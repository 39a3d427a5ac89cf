// sgdmp_platform.hpp -- the device primitives the mixed-precision optimiser kernels use: the launch macro of
// csrc_common/ccnet_device.hpp under this library's name, the 16-byte vector of four floats that an aligned tensor moves in (one
// global_load_dwordx4 / global_store_dwordx4 per lane; eight bf16 values travel in it as four 32-bit words and come out by bit
// casts) and the pointer type of the tensors, whose addresses come out of a table of integers: naming the global address space
// keeps their loads and stores global_ instead of flat_.  The CPU test-suite has a header of the same name under
// tests/emu_sgdmp/; the product never sees it.
#pragma once
#include "../csrc_common/ccnet_device.hpp"

#define SGDMP_LAUNCH CCNET_LAUNCH

namespace sgdmp {

typedef float vec4 __attribute__((ext_vector_type(4)));      // members x, y, z, w; 16-byte aligned

template <class T>
using global_ptr = __attribute__((address_space(1))) T *;

}  // namespace sgdmp
