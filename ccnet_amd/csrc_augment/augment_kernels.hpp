// augment_kernels.hpp -- the one kernel behind include/ccnet_augment.h.
//
//   crop_kernel   one thread per output pixel of one sample (blockIdx.y), consecutive lanes along the crop's rows, so the
//                 three float planes and the int64 label plane are stored coalesced.  The thread maps its pixel back through
//                 the mirror, the crop offset and the scale to four source pixels and one source label, reads them a byte at
//                 a time (3-byte pixels: no load is widened past a pixel, so none can pass the end of a frame or of the
//                 packed buffer) and blends in 32-bit unsigned integers.  Nothing of scaled-frame size exists.  No LDS, no
//                 barrier, no atomics: every output element is written once, by the thread that owns it.
// The arithmetic is the header's, term by term; tests/augment_oracle.py restates it in NumPy int64.
#pragma once
#include <augment_platform.hpp>

#include <stdint.h>

#include "ccnet_augment.h"

namespace augment {

constexpr int kThreads = 256;

struct Tap {                           // one axis of the bilinear footprint: the two source indices and the weight of the second
    int i0, i1;
    unsigned r;                        // in units of 1 / (2 * num)
};

// sx = (o + 1/2) * den / num - 1/2 as i0 + r / (2 * num), clamped to [0, n_src - 1] (o < 65535, den <= 1024: 32 bits suffice)
__device__ __forceinline__ Tap axis_tap(int o, int num, int den, int n_src) {
    Tap t;
    t.i0 = 0;
    t.r = 0u;
    const int s = (2 * o + 1) * den - num;
    if (s > 0) {
        const unsigned D = 2u * (unsigned)num;
        const unsigned q = (unsigned)s / D;
        t.i0 = (int)q;
        t.r = (unsigned)s - q * D;
    }
    if (t.i0 >= n_src - 1) {
        t.i0 = n_src - 1;
        t.r = 0u;
    }
    t.i1 = t.i0 + 1 < n_src ? t.i0 + 1 : n_src - 1;
    return t;
}

// INTER_NEAREST: min(floor(o * den / num), n_src - 1)
__device__ __forceinline__ int nearest(int o, int num, int den, int n_src) {
    const int s = (int)((unsigned)(o * den) / (unsigned)num);
    return s < n_src - 1 ? s : n_src - 1;
}

__global__ __launch_bounds__(kThreads) void crop_kernel(const uint8_t *__restrict__ frames, const uint8_t *__restrict__ labels,
                                                        const int32_t *__restrict__ desc, const uint8_t *__restrict__ table,
                                                        float *__restrict__ images, int64_t *__restrict__ out_labels,
                                                        int crop_h, int crop_w, float mean0, float mean1, float mean2,
                                                        int ignore_label, int source_rgb) {
    const int plane = crop_h * crop_w;
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= plane) return;
    const int b = blockIdx.y;
    const int32_t *d = desc + (size_t)b * CCNET_AUGMENT_DESC_INTS;
    const int Hs = d[CCNET_AUGMENT_HS], Ws = d[CCNET_AUGMENT_WS], pitch = d[CCNET_AUGMENT_PITCH];
    const int num = d[CCNET_AUGMENT_NUM], den = d[CCNET_AUGMENT_DEN];
    const int y = idx / crop_w, x = idx - y * crop_w;
    const int Y = d[CCNET_AUGMENT_H_OFF] + y;
    const int X = d[CCNET_AUGMENT_W_OFF] + (d[CCNET_AUGMENT_MIRROR] ? crop_w - 1 - x : x);

    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    long long lab = ignore_label;
    if (Y < d[CCNET_AUGMENT_HZ] && X < d[CCNET_AUGMENT_WZ]) {
        const Tap ty = axis_tap(Y, num, den, Hs), tx = axis_tap(X, num, den, Ws);
        const uint8_t *f = frames + (size_t)(unsigned)d[CCNET_AUGMENT_FRAME_OFF];
        const uint8_t *p00 = f + ((size_t)ty.i0 * pitch + tx.i0) * 3, *p01 = f + ((size_t)ty.i0 * pitch + tx.i1) * 3;
        const uint8_t *p10 = f + ((size_t)ty.i1 * pitch + tx.i0) * 3, *p11 = f + ((size_t)ty.i1 * pitch + tx.i1) * 3;
        const unsigned D = 2u * (unsigned)num, DD = D * D, half = DD / 2u;
        const unsigned wx1 = tx.r, wx0 = D - tx.r, wy1 = ty.r, wy0 = D - ty.r;
        unsigned q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {                                   // c: the byte within the source pixel
            const unsigned n = ((unsigned)p00[c] * wx0 + (unsigned)p01[c] * wx1) * wy0
                               + ((unsigned)p10[c] * wx0 + (unsigned)p11[c] * wx1) * wy1;
            q[c] = (n + half) / DD;
        }
        // the output is B, G, R: byte 2 - c of an R, G, B source
        v0 = (float)(source_rgb ? q[2] : q[0]) - mean0;
        v1 = (float)q[1] - mean1;
        v2 = (float)(source_rgb ? q[0] : q[2]) - mean2;
        const int sy = nearest(Y, num, den, Hs), sx = nearest(X, num, den, Ws);
        const unsigned v = labels[(size_t)(unsigned)d[CCNET_AUGMENT_LABEL_OFF] + (size_t)sy * pitch + sx];
        lab = table ? table[v] : v;
    }
    float *out = images + (size_t)b * 3 * plane + idx;
    out[0] = v0;
    out[plane] = v1;
    out[2 * (size_t)plane] = v2;
    out_labels[(size_t)b * plane + idx] = lab;
}

}  // namespace augment
