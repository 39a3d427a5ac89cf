// eval_platform.hpp (tests/emu_eval) -- SIMT-emulator implementations of the device primitives of
// ccnet_amd/csrc_eval/eval_platform.hpp, on top of the shared emulator in tests/emu/.  Test infrastructure only: the
// emulator build of the evaluation kernel puts this directory FIRST on the include path; the product build never does.
#pragma once
#include "hip_emu.hpp"

#include <stdint.h>

namespace segeval {

constexpr int kEmuLdsWords = 256 * 256 / 2;   // the largest histogram the kernel asks for (C = 256, two counters a word)

// fibers switch only at barriers and collectives, and workgroups run one after another, so plain adds are atomic here
__device__ inline void lds_add(unsigned *p, unsigned v) { *p += v; }
__device__ inline void global_add(int64_t *p, unsigned v) { *p += (int64_t)v; }

inline int allow_dynamic_lds(const void *, int bytes) { return bytes <= kEmuLdsWords * 4 ? 0 : -1; }

}  // namespace segeval

#define EVAL_DYNAMIC_LDS(name) static unsigned name[segeval::kEmuLdsWords]
#define EVAL_LAUNCH(kern, grid, block, lds_bytes, stream, ...) emu::launch((grid), (block), [&]() { kern(__VA_ARGS__); })
