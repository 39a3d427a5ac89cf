// toy_api.cpp (tests/emu_toy) -- C entry points of the emulator's self-test kernels (toy_kernels.hpp).  Test infrastructure only.
#include "toy_kernels.hpp"

extern "C" {
void toy_ring(const float *src, float *out, int nstage, int variant) {
    CCA_LAUNCH(toy::ring_kernel, dim3(1), dim3(toy::kThreads), nullptr, src, out, nstage, variant);
}
void toy_lane_count(const float *src, float *out, float *sink) {
    CCA_LAUNCH(toy::lane_count_kernel, dim3(1), dim3(cca::kWave), nullptr, src, out, sink);
}
void toy_syncthreads(const float *src, float *out) { CCA_LAUNCH(toy::syncthreads_kernel, dim3(1), dim3(cca::kWave), nullptr, src, out); }
void toy_handover(float *out, int writer, int with_barrier) {
    CCA_LAUNCH(toy::handover_kernel, dim3(1), dim3(toy::kThreads), nullptr, out, writer, with_barrier);
}
void toy_unmergeable(float *sink) { CCA_LAUNCH(toy::unmergeable_kernel, dim3(1), dim3(cca::kWave), nullptr, sink); }
}
