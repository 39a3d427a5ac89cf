// conv3_platform.hpp -- the device primitives of the convolution kernels that csrc/cca_platform.hpp lacks (gfx950 forms).  The CPU
// test-suite has a header of the same name under tests/emu_conv3/ that implements them in the SIMT emulator; the product never
// sees it.
#pragma once
#include <cca_platform.hpp>

namespace conv3 {

typedef unsigned int u32x2v __attribute__((ext_vector_type(2)));

// 8-byte buffer load (two dwords; 4-byte alignment suffices); out-of-range lanes read zeros
__device__ __forceinline__ u32x2v fbuf_load_x2(const cca::FBuf &b, int voff_bytes, int soff_bytes) {
    return __builtin_bit_cast(u32x2v, __builtin_amdgcn_raw_buffer_load_b64(b, voff_bytes, soff_bytes, 0));
}

// The stage barrier of the convolution kernels: csrc/cca_platform.hpp's counted barrier (wait until at most KEEP of this wave's
// vector-memory operations are in flight, then the workgroup barrier) under the library's own name.  tests/test_emu_modes.py holds
// every line of the attention and projection libraries that calls the counted barrier to a late-mode run of THOSE two libraries;
// this library's lines are held to the same condition by its own emulator build, in tests/test_emu_conv3.py.
template <int KEEP> __device__ __forceinline__ void stage_barrier() { cca::barrier_dma_keep<KEEP>(); }

}  // namespace conv3

#define CONV3_LAUNCH(kern, grid, block, stream, ...)                                       \
    do {                                                                                   \
        (void)hipGetLastError();                                                           \
        hipLaunchKernelGGL(kern, (grid), (block), 0, (hipStream_t)(stream), __VA_ARGS__); \
    } while (0)
