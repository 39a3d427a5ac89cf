// proj_platform.hpp -- the device primitives of the projection kernels that csrc/cca_platform.hpp lacks (gfx950 forms).  The CPU
// test-suite has a header of the same name under tests/emu_proj/ that implements them in the SIMT emulator; the product never
// sees it.
#pragma once
#include <cca_platform.hpp>

namespace proj {

typedef unsigned int u32x2v __attribute__((ext_vector_type(2)));

// 8-byte buffer load (two dwords; 4-byte alignment suffices); out-of-range lanes read zeros
__device__ __forceinline__ u32x2v fbuf_load_x2(const cca::FBuf &b, int voff_bytes, int soff_bytes) {
    return __builtin_bit_cast(u32x2v, __builtin_amdgcn_raw_buffer_load_b64(b, voff_bytes, soff_bytes, 0));
}

}  // namespace proj

#define PROJ_LAUNCH(kern, grid, block, stream, ...)                                        \
    do {                                                                                   \
        (void)hipGetLastError();                                                           \
        hipLaunchKernelGGL(kern, (grid), (block), 0, (hipStream_t)(stream), __VA_ARGS__); \
    } while (0)
