// conv3_platform.hpp (tests/emu_conv3) -- SIMT-emulator twins of ccnet_amd/csrc_conv3/conv3_platform.hpp.  Test infrastructure
// only: the emulator build puts tests/emu and this directory FIRST on the include path; the product build never does.
#pragma once
#include <cca_platform.hpp>

namespace conv3 {

typedef unsigned int u32x2v __attribute__((ext_vector_type(2)));

__device__ inline u32x2v fbuf_load_x2(const cca::FBuf &b, int voff_bytes, int soff_bytes, CCA_EMU_SITE) {
    emu::vmem_note(site, site_file);                 // one vector-memory instruction
    u32x2v v;
    for (int e = 0; e < 2; ++e) {
        const float f = cca::emu_fbuf_get(b, voff_bytes + 4 * e, soff_bytes);
        uint32_t u;
        memcpy(&u, &f, 4);
        v[e] = u;
    }
    return v;
}

// (the barrier is charged to the line of the kernel that calls it)
template <int KEEP> __device__ inline void stage_barrier(CCA_EMU_SITE) { cca::barrier_dma_keep<KEEP>(site, site_file); }

}  // namespace conv3

#define CONV3_LAUNCH(kern, grid, block, stream, ...) emu::launch((grid), (block), [&]() { kern(__VA_ARGS__); })
