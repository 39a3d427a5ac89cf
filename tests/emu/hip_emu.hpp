// hip_emu.hpp -- a tiny host-side SIMT emulator used ONLY by the CPU test-suite.
//
// The build container has no GPU, so the kernels in ccnet_amd/csrc/ would otherwise first execute
// on the (scarce) MI355X box.  This shim lets the *same kernel source* be compiled by the host
// clang++ and executed on the CPU: every HIP thread of a workgroup is a fiber; __syncthreads(),
// wave shuffles and the f32 MFMA are rendez-vous points between fibers.  Fibers run until they
// block, so a missing barrier shows up as a wrong answer -- in ONE direction of each race.  The scheduler visits the threads
// in ascending order, so a low wavefront has always run before a high one: a low wave reading what a high wave has yet to
// write is seen; a high wave reading too early what a low wave writes, or overwriting too early what a low wave reads, is not.
// CCA_EMU_REVERSE=1 visits wavefronts, and lanes within them, in descending order and sees exactly the other half.  LDS is
// poisoned with NaNs per workgroup, and LDS bank conflicts of ds_read/ds_write_b32 are counted.
//
// CCA_EMU_LATE_DMA=1 models the vector-memory queue: every wavefront keeps its outstanding vector-memory
// instructions in order, an LDS-DMA lands in LDS only when a wait retires it, and the counted barriers retire exactly what
// their count allows -- the latest moment the device may complete it.  CCA_EMU_KEEP_PLUS=1 adds one to every count (the
// tests' proof that a count one too high is seen).  All three are read by emu::launch; unset, nothing changes.
//
// It is test infrastructure: nothing in the product (ccnet_amd/, cc_attention/) links or loads it,
// and the library it produces (tests/emu/libcca_emu.so) is never on the GPU path.
#pragma once
#ifndef CCNET_EMU
#define CCNET_EMU 1
#endif

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};

typedef void *hipStream_t;
typedef int hipError_t;
#define hipSuccess 0
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipPeekAtLastError() { return 0; }
inline const char *hipGetErrorString(hipError_t) { return "emu"; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
enum { hipMemcpyDeviceToHost = 2 };
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { std::memcpy(d, s, n); return 0; }
inline hipError_t hipMemcpy(void *d, const void *s, size_t n, int) { std::memcpy(d, s, n); return 0; }

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
#define __launch_bounds__(...)
#define __shared__ static

namespace emu {

struct Lane {
    dim3 tid;
};
extern dim3 g_block, g_bdim, g_gdim;
extern Lane *g_cur;

void launch(dim3 grid, dim3 block, const std::function<void()> &body);
// what a workgroup barrier does to the calling wave's vector-memory queue (late mode)
enum Barrier {
    BAR_SYNC,        // __syncthreads(): retires up to and including the youngest LDS-DMA the compiler can see
    BAR_LDS_ONLY,    // retires nothing
    BAR_KEEP         // retires all but the youngest `keep` instructions
};
void block_barrier(int kind = BAR_SYNC, int keep = 0, int line = 0, const char *file = nullptr);
// late mode: the vector-memory queue of the calling lane's wave
extern bool g_late;
void vmem_note(int line, const char *file);                    // a load or a store: takes effect at once, occupies a slot
// an LDS-DMA: `ndw` dwords of this lane, captured now, written to dst_wave_base[lane_dword_off ...] when retired
void vmem_dma(int line, const char *file, float *dst_wave_base, int lane_dword_off, const float *data, int ndw, bool compiler_visible);
void vmem_wait_all();                                          // s_waitcnt vmcnt(0): wave-collective
void set_barrier_site(int line, const char *file);             // the source line the lane's next counted barrier is charged to
// exchange one 64-bit payload per lane across the calling lane's wave; returns pointer to the
// wave's 64 payload slots (valid until the lane's next collective).
const uint64_t *wave_exchange(uint64_t mine);
// wider payloads: up to 32 bytes per lane; returns the wave's 64 slots of 32 bytes each
const unsigned char *wave_exchange_bytes(const void *mine, size_t nbytes);
int lane_id();

// LDS instrumentation: kernels register their __shared__ array so it can be poisoned and so
// that bank conflicts of 4-byte accesses can be counted per wave-instruction.
void lds_register(void *base, size_t bytes);
void lds_note_read(const void *addr, int site);
void lds_note_write(const void *addr, int site);
struct Stats {
    unsigned long long lds_read_instr, lds_read_cycles, lds_write_instr, lds_write_cycles, mfma, launches;
};
Stats &stats();

}  // namespace emu

#define threadIdx (emu::g_cur->tid)
#define blockIdx (emu::g_block)
#define blockDim (emu::g_bdim)
#define gridDim (emu::g_gdim)
inline void __syncthreads() { emu::block_barrier(); }
