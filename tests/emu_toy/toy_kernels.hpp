// toy_kernels.hpp (tests/emu_toy) -- toy kernels that test the SIMT emulator itself (tests/test_emu_model.py): its late-landing
// vector-memory model and its reversed schedule.  Test infrastructure only: built into tests/emu_toy/libtoy_emu.so
// and nowhere else, and written with the platform primitives of <cca_platform.hpp> alone.  Every kernel is one workgroup.
#pragma once
#include <cca_platform.hpp>

namespace toy {

using namespace cca;

constexpr int kThreads = 128;             // two wavefronts
constexpr float kSentinel = -1.f;         // what an LDS slot holds before its fill lands

template <int KEEP_MAX>
__device__ inline void keep_n(int n);
template <>
__device__ inline void keep_n<0>(int) { barrier_dma_keep<0>(); }
template <>
__device__ inline void keep_n<3>(int n) {
    if (n <= 0)      barrier_dma_keep<0>();
    else if (n == 1) barrier_dma_keep<1>();
    else if (n == 2) barrier_dma_keep<2>();
    else             barrier_dma_keep<3>();
}

// A two-deep LDS-DMA ring.  Stage s is 128 floats of src; each wave fills its own half of a slot and reads the OTHER wave's half,
// then stores it to out.  At the hand-over barrier of step s the wave's queue holds, oldest first: fill(s), the store of step
// s - 1 (s > 0), fill(s + 1) (s + 1 < nstage) -- fill(s) has landed when at most (s > 0) + (s + 1 < nstage) are kept.
//   variant 0: that count;  1: one more;  2: barrier_lds_only() in its place
enum { RING_RIGHT = 0, RING_KEEP_PLUS_ONE = 1, RING_LDS_ONLY = 2 };
__global__ void ring_kernel(const float *src, float *out, int nstage, int variant) {
    __shared__ float ring[2][kThreads];
    CCA_LDS_REGISTER(ring);
    const int tid = threadIdx.x, wv = tid / kWave;
    const FBuf sb = make_fbuf(src, size_t(nstage) * kThreads * 4), ob = make_fbuf(out, size_t(nstage) * kThreads * 4);
    fbuf_load_to_lds(sb, ring[0] + wv * kWave, tid * 4, 0);
    for (int s = 0; s < nstage; ++s) {
        if (s + 1 < nstage)
            fbuf_load_to_lds(sb, ring[(s + 1) & 1] + wv * kWave, tid * 4, (s + 1) * kThreads * 4);
        const int keep = (s > 0) + (s + 1 < nstage);
        if (variant == RING_LDS_ONLY) barrier_lds_only();
        else                          keep_n<3>(keep + (variant == RING_KEEP_PLUS_ONE));
        const float v = CCA_LDS_LD(&ring[s & 1][(tid + kWave) % kThreads]);
        fbuf_store(ob, v, tid * 4, s * kThreads * 4);
        barrier_lds_only();                               // every wave is done with slot s & 1 before step s + 1 refills it
    }
}

// One wave instruction is one slot, however many lanes issue it; an instruction no lane issues is none.  Two fills X and Y, a
// store that only the odd lanes issue, a store that no lane issues, then keep<2>: X has landed and Y has not, if and only if the
// two stores together count exactly once.  out[0..63]: X's slot, out[64..127]: Y's slot after that barrier; out[128..191]: Y's slot
// after wait_vmem_all().  One wave of 64 threads.
__global__ void lane_count_kernel(const float *src, float *out, float *sink) {
    __shared__ float slot[2][kWave];
    CCA_LDS_REGISTER(slot);
    const int l = threadIdx.x;
    const FBuf sb = make_fbuf(src, 2 * kWave * 4), kb = make_fbuf(sink, kWave * 4);
    CCA_LDS_ST(&slot[0][l], kSentinel);
    CCA_LDS_ST(&slot[1][l], kSentinel);
    barrier_lds_only();
    fbuf_load_to_lds(sb, slot[0], l * 4, 0);                        // X
    fbuf_load_to_lds(sb, slot[1], l * 4, kWave * 4);                // Y
    if (l & 1) fbuf_store(kb, 1.f, l * 4, 0);                       // divergent: one instruction
    if (l >= kWave) fbuf_store(kb, 2.f, l * 4, 0);                  // no lane: no instruction
    barrier_dma_keep<2>();
    out[l] = CCA_LDS_LD(&slot[0][l]);
    out[kWave + l] = CCA_LDS_LD(&slot[1][l]);
    wait_vmem_all();
    out[2 * kWave + l] = CCA_LDS_LD(&slot[1][l]);
}

// __syncthreads() waits for the LDS-DMAs the compiler sees, and so for everything older than the youngest of them; an uncounted
// fill issued after it stays in flight.  barrier_lds_only() waits for nothing; the end of the kernel for everything.
// out[0..63]: the visible fill's slot, out[64..127]: the uncounted fill's slot after __syncthreads(); out[128..191] / out[192..255]:
// the same after a barrier_lds_only() that follows.  One wave.
__global__ void syncthreads_kernel(const float *src, float *out) {
    __shared__ float slot[2][kWave];
    CCA_LDS_REGISTER(slot);
    const int l = threadIdx.x;
    const FBuf sb = make_fbuf(src, 2 * kWave * 4);
    CCA_LDS_ST(&slot[0][l], kSentinel);
    CCA_LDS_ST(&slot[1][l], kSentinel);
    barrier_lds_only();
    fbuf_load_to_lds(sb, slot[0], l * 4, 0);
    if (l < 16) fbuf_load_to_lds_x4_uncounted(sb, slot[1], (kWave + 4 * l) * 4);       // 16 lanes x 4 dwords = the slot
    __syncthreads();
    out[l] = CCA_LDS_LD(&slot[0][l]);
    out[kWave + l] = CCA_LDS_LD(&slot[1][l]);
    barrier_lds_only();
    out[2 * kWave + l] = CCA_LDS_LD(&slot[0][l]);
    out[3 * kWave + l] = CCA_LDS_LD(&slot[1][l]);
}

// A hand-over between two waves through LDS with its barrier left out (with_barrier = 0).  Wave `writer` writes, the other reads.
// The scheduler runs every thread until it blocks, in ascending order: writer = 0 then looks right, writer = 1 reads the poison;
// in descending order it is the other way round.  out[0..63]: what the reading wave saw.
__global__ void handover_kernel(float *out, int writer, int with_barrier) {
    __shared__ float box[kWave];
    CCA_LDS_REGISTER(box);
    const int tid = threadIdx.x, wv = tid / kWave, l = tid % kWave;
    if (wv == writer) CCA_LDS_ST(&box[l], float(100 + l));
    if (with_barrier) barrier_lds_only();
    if (wv != writer) out[l] = CCA_LDS_LD(&box[(l + 1) % kWave]);
}

// The lanes of one wave issue different stores on the two sides of a branch: neither side's sequence contains the other's, the
// source does not say how many instructions the device issues for them nor in which order, and a counted barrier that has to
// count them makes the emulator stop (late mode) and name a line of this branch.  (keep<0> would not: it retires them whole.)
__global__ void unmergeable_kernel(float *sink) {
    const int l = threadIdx.x;
    const FBuf kb = make_fbuf(sink, kWave * 4);
    if (l < 32) fbuf_store(kb, 1.f, l * 4, 0);                      // UNMERGEABLE-A
    else        fbuf_store(kb, 2.f, l * 4, 0);                      // UNMERGEABLE-B
    barrier_dma_keep<1>();
}

}  // namespace toy
