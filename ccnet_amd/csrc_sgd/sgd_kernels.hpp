// sgd_kernels.hpp -- the two kernels behind include/ccnet_sgd.h.
//
//   step_kernel      one workgroup per chunk of CCNET_SGD_CHUNK elements of one tensor, the grid striding over the chunk table.
//                    The chunk's table row, the tensor's row and the group's hyper-parameters are the same for every lane, so
//                    the choice between the 16-byte path and the element path never splits a wave.  A lane loads kBatch
//                    vectors (or elements) of p, g and b before it uses the first, updates them and stores p, b and, when
//                    asked to, a zeroed g: every element is read once and written once, 24 bytes per parameter.  No LDS, no
//                    barrier, no atomics.
//   advance_kernel   one thread: *counter += 1, launched behind step_kernel on the same stream, so every workgroup of a step
//                    has read the same value.
// The arithmetic is the header's, operation by operation, with contraction into fused multiply-adds switched off;
// tests/sgd_oracle.py restates it in NumPy float32.
#pragma once
#include <sgd_platform.hpp>

#include <stdint.h>

#include "ccnet_sgd.h"

namespace sgd {

constexpr int kThreads = 256;
constexpr int kBatch = 4;                      // loads of each of p, g, b in flight per lane
static_assert(CCNET_SGD_CHUNK % (4 * kThreads) == 0, "a chunk is whole 16-byte rounds of the workgroup");

struct Hyper {                                 // by value in the kernel's arguments: no copy to the device per step
    float lr[CCNET_SGD_MAX_GROUPS], wd[CCNET_SGD_MAX_GROUPS], mu[CCNET_SGD_MAX_GROUPS];
};

// one element: d = g + wd p; b' = mu b + d; p' = p - lr b', every operation rounded on its own
__device__ __forceinline__ void update(float &p, float g, float &b, float lr, float wd, float mu) {
#pragma clang fp contract(off)
    const float wp = wd * p;
    const float d = g + wp;
    const float mb = mu * b;
    const float nb = mb + d;
    const float step = lr * nb;
    p = p - step;
    b = nb;
}

// (component by component through floats of its own: a vector's member does not bind to a reference)
#define SGD_COMPONENT(c)                   \
    {                                      \
        float pc = p.c, bc = b.c;          \
        update(pc, g.c, bc, lr, wd, mu);   \
        p.c = pc;                          \
        b.c = bc;                          \
    }
__device__ __forceinline__ void update(vec4 &p, const vec4 &g, vec4 &b, float lr, float wd, float mu) {
    SGD_COMPONENT(x)
    SGD_COMPONENT(y)
    SGD_COMPONENT(z)
    SGD_COMPONENT(w)
}
#undef SGD_COMPONENT

__device__ __forceinline__ void clear(float &v) { v = 0.f; }
__device__ __forceinline__ void clear(vec4 &v) { v.x = v.y = v.z = v.w = 0.f; }

// kBatch rounds of the workgroup from element (or vector) `base`; FULL: all of them lie below n
template <bool FULL, class T>
__device__ __forceinline__ void rounds(global_ptr<T> p, global_ptr<T> g, global_ptr<T> b, int base, int n, float lr, float wd,
                                       float mu, bool zero) {
    T vp[kBatch], vg[kBatch], vb[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
        const int i = base + j * kThreads + (int)threadIdx.x;
        if (FULL || i < n) {
            vp[j] = p[i];
            vg[j] = g[i];
            vb[j] = b[i];
        }
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
        const int i = base + j * kThreads + (int)threadIdx.x;
        if (FULL || i < n) {
            update(vp[j], vg[j], vb[j], lr, wd, mu);
            p[i] = vp[j];
            b[i] = vb[j];
            if (zero) {
                clear(vg[j]);
                g[i] = vg[j];
            }
        }
    }
}

// n elements (or vectors) of one chunk, n <= CCNET_SGD_CHUNK
template <class T>
__device__ __forceinline__ void sweep(global_ptr<T> p, global_ptr<T> g, global_ptr<T> b, int n, float lr, float wd, float mu,
                                      bool zero) {
    constexpr int kRound = kBatch * kThreads;
    int base = 0;
    for (; base + kRound <= n; base += kRound) rounds<true, T>(p, g, b, base, n, lr, wd, mu, zero);
    if (base < n) rounds<false, T>(p, g, b, base, n, lr, wd, mu, zero);
}

__global__ __launch_bounds__(kThreads) void step_kernel(const int64_t *__restrict__ tensors, const int32_t *__restrict__ chunks,
                                                        int n_chunks, Hyper h, const float *__restrict__ schedule,
                                                        int schedule_len, const int32_t *__restrict__ counter, int zero_grads) {
    float table_lr = 0.f;
    if (schedule) {
        int s = *counter;
        s = s < 0 ? 0 : s;
        table_lr = schedule[s < schedule_len - 1 ? s : schedule_len - 1];
    }
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int32_t t = chunks[2 * (size_t)c], k = chunks[2 * (size_t)c + 1];
        const int64_t *row = tensors + (size_t)t * CCNET_SGD_TENSOR_WORDS;
        const uintptr_t pa = (uintptr_t)row[CCNET_SGD_P], ga = (uintptr_t)row[CCNET_SGD_G], ba = (uintptr_t)row[CCNET_SGD_B];
        if (!ga) continue;                                            // no gradient: p and b stay as they are
        const int group = (int)row[CCNET_SGD_GROUP];
        float lr = h.lr[0], wd = h.wd[0], mu = h.mu[0];
#pragma unroll
        for (int q = 1; q < CCNET_SGD_MAX_GROUPS; ++q) {              // (constant indices: the argument block is never addressed by a register)
            if (group == q) {
                lr = h.lr[q];
                wd = h.wd[q];
                mu = h.mu[q];
            }
        }
        if (schedule) lr = table_lr * lr;
        const int64_t first = (int64_t)k * CCNET_SGD_CHUNK;           // below numel <= 2^31 - 1
        const int64_t left = row[CCNET_SGD_NUMEL] - first;
        const int len = left < CCNET_SGD_CHUNK ? (int)left : CCNET_SGD_CHUNK;
        const global_ptr<float> p = reinterpret_cast<global_ptr<float>>(pa) + first;
        const global_ptr<float> g = reinterpret_cast<global_ptr<float>>(ga) + first;
        const global_ptr<float> b = reinterpret_cast<global_ptr<float>>(ba) + first;
        const bool zero = zero_grads != 0;
        if (((pa | ga | ba) & 15) == 0) {                             // per tensor (a chunk starts a multiple of 16 bytes in)
            const int nv = len >> 2;
            sweep<vec4>(reinterpret_cast<global_ptr<vec4>>(p), reinterpret_cast<global_ptr<vec4>>(g),
                        reinterpret_cast<global_ptr<vec4>>(b), nv, lr, wd, mu, zero);
            const int i = 4 * nv + (int)threadIdx.x;                  // the tensor's last numel % 4 elements
            if (i < len) {
                float vp = p[i], vb = b[i];
                update(vp, g[i], vb, lr, wd, mu);
                p[i] = vp;
                b[i] = vb;
                if (zero) g[i] = 0.f;
            }
        } else {
            sweep<float>(p, g, b, len, lr, wd, mu, zero);
        }
    }
}

__global__ void advance_kernel(int32_t *counter) {
    const int32_t s = *counter;
    *counter = s < 0x7fffffff ? s + 1 : s;
}

}  // namespace sgd
