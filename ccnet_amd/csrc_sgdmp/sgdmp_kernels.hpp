// sgdmp_kernels.hpp -- the two kernels behind include/ccnet_sgdmp.h.
//
//   step_kernel      one workgroup per chunk of CCNET_SGD_CHUNK elements of one tensor, the grid striding over the chunk table.
//                    The chunk's table row, the tensor's row and the group's hyper-parameters are the same for every lane, so
//                    the choice between the kinds of row and between the 16-byte path and the element path never splits a wave.
//                      master row (M != 0)   a lane takes eight elements per round: one 16-byte vector of g (eight bf16), two
//                                            each of the float32 m and b; it loads kBatchMaster rounds of them before it uses
//                                            the first, updates m and b, rounds m to bf16 and stores two vectors each of m and
//                                            b, one of p and, when asked to, one zeroed g: 22 bytes per parameter, p never read.
//                                            The tensor's last numel % 8 elements, and a tensor off 16 bytes, go by element.
//                      float32 row (M == 0)  csrc_sgd/sgd_kernels.hpp's sweep, restated: 24 bytes per parameter.
//                    No LDS, no barrier, no atomics.
//   advance_kernel   one thread: *counter += 1, launched behind step_kernel on the same stream, so every workgroup of a step
//                    has read the same value.
// The arithmetic is the header's, operation by operation, with contraction into fused multiply-adds switched off; the bf16
// halves come out of and go into the 16-byte vector by bit casts, and the rounding to bf16 is integer arithmetic, so the
// device, the emulator build and tests/sgdmp_oracle.py agree bit for bit.
#pragma once
#include <sgdmp_platform.hpp>

#include <stdint.h>

#include "ccnet_sgdmp.h"

namespace sgdmp {

constexpr int kThreads = 256;
constexpr int kBatch = 4;                      // float32 rows: loads of each of p, g, b in flight per lane
constexpr int kBatchMaster = 2;                // master rows: rounds in flight per lane, five 16-byte loads each
static_assert(CCNET_SGD_CHUNK % (8 * kThreads * kBatchMaster) == 0, "a full chunk is whole rounds of the workgroup on either path");

struct Hyper {                                 // by value in the kernel's arguments: no copy to the device per step
    float lr[CCNET_SGD_MAX_GROUPS], wd[CCNET_SGD_MAX_GROUPS], mu[CCNET_SGD_MAX_GROUPS];
};

__device__ __forceinline__ uint32_t bits_of(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, sizeof u);
    return u;
}

__device__ __forceinline__ float float_of(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, sizeof f);
    return f;
}

// float32 -> bf16, to nearest, ties to even, on the bit pattern; a NaN stays one
__device__ __forceinline__ uint32_t bf16_rne(float f) {
    const uint32_t u = bits_of(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// one element: d = g + wd p; b' = mu b + d; p' = p - lr b', every operation rounded on its own (p is the master in a master row)
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
#define SGDMP_COMPONENT(c)                 \
    {                                      \
        float pc = p.c, bc = b.c;          \
        update(pc, g.c, bc, lr, wd, mu);   \
        p.c = pc;                          \
        b.c = bc;                          \
    }
__device__ __forceinline__ void update(vec4 &p, const vec4 &g, vec4 &b, float lr, float wd, float mu) {
    SGDMP_COMPONENT(x)
    SGDMP_COMPONENT(y)
    SGDMP_COMPONENT(z)
    SGDMP_COMPONENT(w)
}
#undef SGDMP_COMPONENT

__device__ __forceinline__ void clear(float &v) { v = 0.f; }
__device__ __forceinline__ void clear(vec4 &v) { v.x = v.y = v.z = v.w = 0.f; }

// ---- float32 rows: sgd_kernels.hpp's rounds and sweep ----------------------------------------------------------------------

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

// ---- master rows -----------------------------------------------------------------------------------------------------------

// two elements: the bf16 pair in the 32-bit word `g` (the lower address in the lower half) against m0, m1 and b0, b1; returns
// the pair bf16(m0'), bf16(m1') as one word
__device__ __forceinline__ float pair(float g, float &m0, float &m1, float &b0, float &b1, float lr, float wd, float mu) {
    const uint32_t u = bits_of(g);
    update(m0, float_of(u << 16), b0, lr, wd, mu);
    update(m1, float_of(u & 0xffff0000u), b1, lr, wd, mu);
    return float_of(bf16_rne(m0) | (bf16_rne(m1) << 16));
}

// eight elements: g's eight bf16 against (ma, mb) and (ba, bb); returns the eight bf16 of p
__device__ __forceinline__ vec4 update8(const vec4 &g, vec4 &ma, vec4 &mb, vec4 &ba, vec4 &bb, float lr, float wd, float mu) {
    float m[8] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
    float b[8] = {ba.x, ba.y, ba.z, ba.w, bb.x, bb.y, bb.z, bb.w};
    vec4 p;
    p.x = pair(g.x, m[0], m[1], b[0], b[1], lr, wd, mu);
    p.y = pair(g.y, m[2], m[3], b[2], b[3], lr, wd, mu);
    p.z = pair(g.z, m[4], m[5], b[4], b[5], lr, wd, mu);
    p.w = pair(g.w, m[6], m[7], b[6], b[7], lr, wd, mu);
    ma.x = m[0], ma.y = m[1], ma.z = m[2], ma.w = m[3], mb.x = m[4], mb.y = m[5], mb.z = m[6], mb.w = m[7];
    ba.x = b[0], ba.y = b[1], ba.z = b[2], ba.w = b[3], bb.x = b[4], bb.y = b[5], bb.z = b[6], bb.w = b[7];
    return p;
}

// kBatchMaster rounds of the workgroup from group-of-eight `base`; FULL: all of them lie below n.  p and g hold one vector per
// group of eight, m and b two.
template <bool FULL>
__device__ __forceinline__ void master_rounds(global_ptr<vec4> p, global_ptr<vec4> g, global_ptr<vec4> m, global_ptr<vec4> b,
                                              int base, int n, float lr, float wd, float mu, bool zero) {
    vec4 vg[kBatchMaster], vm[kBatchMaster][2], vb[kBatchMaster][2];
#pragma unroll
    for (int j = 0; j < kBatchMaster; ++j) {
        const int i = base + j * kThreads + (int)threadIdx.x;
        if (FULL || i < n) {
            vg[j] = g[i];
            vm[j][0] = m[2 * i];
            vm[j][1] = m[2 * i + 1];
            vb[j][0] = b[2 * i];
            vb[j][1] = b[2 * i + 1];
        }
    }
#pragma unroll
    for (int j = 0; j < kBatchMaster; ++j) {
        const int i = base + j * kThreads + (int)threadIdx.x;
        if (FULL || i < n) {
            const vec4 vp = update8(vg[j], vm[j][0], vm[j][1], vb[j][0], vb[j][1], lr, wd, mu);
            m[2 * i] = vm[j][0];
            m[2 * i + 1] = vm[j][1];
            b[2 * i] = vb[j][0];
            b[2 * i + 1] = vb[j][1];
            p[i] = vp;
            if (zero) {
                clear(vg[j]);
                g[i] = vg[j];
            }
        }
    }
}

// n groups of eight elements of one chunk, n <= CCNET_SGD_CHUNK / 8
__device__ __forceinline__ void master_sweep(global_ptr<vec4> p, global_ptr<vec4> g, global_ptr<vec4> m, global_ptr<vec4> b, int n,
                                             float lr, float wd, float mu, bool zero) {
    constexpr int kRound = kBatchMaster * kThreads;
    int base = 0;
    for (; base + kRound <= n; base += kRound) master_rounds<true>(p, g, m, b, base, n, lr, wd, mu, zero);
    if (base < n) master_rounds<false>(p, g, m, b, base, n, lr, wd, mu, zero);
}

// elements [from, n) of one chunk one by one, the workgroup striding over them
__device__ __forceinline__ void master_elements(global_ptr<uint16_t> p, global_ptr<uint16_t> g, global_ptr<float> m,
                                                global_ptr<float> b, int from, int n, float lr, float wd, float mu, bool zero) {
    for (int i = from + (int)threadIdx.x; i < n; i += kThreads) {
        float vm = m[i], vb = b[i];
        update(vm, float_of((uint32_t)g[i] << 16), vb, lr, wd, mu);
        m[i] = vm;
        b[i] = vb;
        p[i] = (uint16_t)bf16_rne(vm);
        if (zero) g[i] = (uint16_t)0;
    }
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
        const int64_t *row = tensors + (size_t)t * CCNET_SGDMP_TENSOR_WORDS;
        const uintptr_t pa = (uintptr_t)row[CCNET_SGDMP_P], ga = (uintptr_t)row[CCNET_SGDMP_G], ba = (uintptr_t)row[CCNET_SGDMP_B];
        const uintptr_t ma = (uintptr_t)row[CCNET_SGDMP_M];
        if (!ga) continue;                                            // no gradient: p, m and b stay as they are
        const int group = (int)row[CCNET_SGDMP_GROUP];
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
        const int64_t left = row[CCNET_SGDMP_NUMEL] - first;
        const int len = left < CCNET_SGD_CHUNK ? (int)left : CCNET_SGD_CHUNK;
        const bool zero = zero_grads != 0;
        const global_ptr<float> b = reinterpret_cast<global_ptr<float>>(ba) + first;
        if (ma) {
            const global_ptr<uint16_t> p = reinterpret_cast<global_ptr<uint16_t>>(pa) + first;
            const global_ptr<uint16_t> g = reinterpret_cast<global_ptr<uint16_t>>(ga) + first;
            const global_ptr<float> m = reinterpret_cast<global_ptr<float>>(ma) + first;
            int done = 0;
            if (((pa | ga | ma | ba) & 15) == 0) {                    // per tensor (a chunk starts a multiple of 16 bytes in, in bf16 too)
                const int nv = len >> 3;
                master_sweep(reinterpret_cast<global_ptr<vec4>>(p), reinterpret_cast<global_ptr<vec4>>(g),
                             reinterpret_cast<global_ptr<vec4>>(m), reinterpret_cast<global_ptr<vec4>>(b), nv, lr, wd, mu, zero);
                done = 8 * nv;                                        // the tensor's last numel % 8 elements follow
            }
            master_elements(p, g, m, b, done, len, lr, wd, mu, zero);
        } else {
            const global_ptr<float> p = reinterpret_cast<global_ptr<float>>(pa) + first;
            const global_ptr<float> g = reinterpret_cast<global_ptr<float>>(ga) + first;
            if (((pa | ga | ba) & 15) == 0) {
                const int nv = len >> 2;
                sweep<vec4>(reinterpret_cast<global_ptr<vec4>>(p), reinterpret_cast<global_ptr<vec4>>(g),
                            reinterpret_cast<global_ptr<vec4>>(b), nv, lr, wd, mu, zero);
                const int i = 4 * nv + (int)threadIdx.x;              // the tensor's last numel % 4 elements
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
}

__global__ void advance_kernel(int32_t *counter) {
    const int32_t s = *counter;
    *counter = s < 0x7fffffff ? s + 1 : s;
}

}  // namespace sgdmp
