// mseval_kernels.hpp -- the two kernels behind include/ccnet_mseval.h (multi-scale evaluation).
//
//   tiles        grid (tile pixel blocks, count, N), 256 threads, one tile position a thread, the Cin channels in a loop
//                (consecutive threads on consecutive columns of a tile row: every store is coalesced).  It fuses the zoom
//                of the image to (Hs, Ws), the mirror along W, the cut and the zero padding: the position's place in the
//                scaled (and, for a flipped tile, mirrored) frame, its exact-ratio taps in the original image, the <= 4 reads
//                and the lerps.  The scaled image is never written.
//   accumulate   grid (pixel blocks, N), 256 threads, 4096 pixels of the (H, W) output a workgroup, as sliding_kernel.  Per
//                pixel: its exact-ratio taps in the scaled frame; per class the per-scale score at the <= 4 tap positions
//                with sliding_kernel's arithmetic (eval_sample.hpp), the lerps, + score_in, / divide_by; optional score,
//                first maximum, and sliding_kernel's LDS histogram of 16-bit counters flushed with integer atomics.
//                Neither the up-sampled tiles nor the per-scale (Hs, Ws) map is materialised.
//
// A tap whose weight is exactly 0 is not read, so at Hs == H, Ws == W the accumulate kernel evaluates one position a pixel
// and gives sliding_kernel's score bit for bit, and the tiles kernel copies.  That rule is the resample's (axis_tap's taps);
// inside a tile, sample() of eval_sample.hpp sums its four terms unconditionally, as PyTorch does.
#pragma once
#include "eval_sample.hpp"

namespace mseval {

using segeval::covers;
using segeval::first_maximum;
using segeval::Geometry;
using segeval::global_add;
using segeval::kPixPerBlock;
using segeval::kPixPerThread;
using segeval::kThreads;
using segeval::lds_add;
using segeval::pass_mean;
using segeval::TileGrid;

struct TilesGeometry {
    int Cin, H, W, Hs, Ws, T, tile_H, tile_W, first, count;
};

struct Axis {                      // the two taps of one output index and the weight of the second
    int i0, i1;
    float l;
};

// ndimage.zoom's coordinate o * (n_in - 1) / (n_out - 1) of output index o, in integers (o < n_out <= 2^31 - 1)
__device__ __forceinline__ Axis axis_tap(int o, int n_in, int n_out) {
    Axis a = {0, 0, 0.f};
    if (n_out > 1) {
        const unsigned long long p = (unsigned long long)(unsigned)o * (unsigned)(n_in - 1);
        const unsigned d = (unsigned)(n_out - 1);
        a.i0 = (int)(p / d);
        a.l = (float)(unsigned)(p % d) / (float)d;
        a.i1 = a.i0 + 1 < n_in ? a.i0 + 1 : n_in - 1;
    }
    return a;
}

// the lerp of two taps whose second weight l is not 0 (the callers do not read b when it is)
__device__ __forceinline__ float lerp(float a, float b, float l) { return (1.f - l) * a + l * b; }

__global__ __launch_bounds__(kThreads) void tiles_kernel(const float *image, TileGrid g, TilesGeometry Q, float *out) {
    const unsigned tile_px = (unsigned)(Q.tile_H * Q.tile_W);
    const unsigned p = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if (p >= tile_px) return;
    const int k = blockIdx.y, n = blockIdx.z;
    const int e = Q.first + k;
    const bool flipped = e >= Q.T;
    const int t = flipped ? e - Q.T : e;
    const int ly = (int)(p / (unsigned)Q.tile_W), lx = (int)(p - (unsigned)ly * (unsigned)Q.tile_W);
    const int y1 = g.y1[t], x1 = g.x1[t];
    const bool inside = ly < Q.Hs - y1 && lx < Q.Ws - x1;               // else: the zero padding of pad_image
    Axis ay = {0, 0, 0.f}, ax = {0, 0, 0.f};
    if (inside) {
        const int xs = x1 + lx;
        ay = axis_tap(y1 + ly, Q.H, Q.Hs);
        ax = axis_tap(flipped ? Q.Ws - 1 - xs : xs, Q.W, Q.Ws);
    }
    const size_t HW = (size_t)Q.H * Q.W;
    float *o = out + ((size_t)n * Q.count + k) * Q.Cin * tile_px + p;
    const float *plane = image + (size_t)n * Q.Cin * HW;
    for (int c = 0; c < Q.Cin; ++c, plane += HW, o += tile_px) {
        float v = 0.f;
        if (inside) {
            const float *r0 = plane + (size_t)ay.i0 * Q.W;
            v = r0[ax.i0];
            if (ax.l != 0.f) v = lerp(v, r0[ax.i1], ax.l);
            if (ay.l != 0.f) {
                const float *r1 = plane + (size_t)ay.i1 * Q.W;
                float b = r1[ax.i0];
                if (ax.l != 0.f) b = lerp(b, r1[ax.i1], ax.l);
                v = lerp(v, b, ay.l);
            }
        }
        *o = v;
    }
}

struct Cover {                     // how many tiles of the plain / the flipped pass cover one position of the scaled frame
    int cnt, cntf;
};

__device__ __forceinline__ Cover cover_counts(const TileGrid &g, const Geometry &G, int y, int x) {
    Cover k = {0, 0};
    const int xf = G.W - 1 - x;
    for (int t = 0; t < G.T; ++t) {
        k.cnt += covers(g, G, t, y, x);
        k.cntf += covers(g, G, t, y, xf);
    }
    return k;
}

// the per-scale score S_s of class c at (y, x) of the scaled frame: sliding_kernel's expression
__device__ __forceinline__ float scaled_score(const float *img, const TileGrid &g, const Geometry &G, int c, int y, int x,
                                              Cover k) {
    float s = 0.f;
#pragma unroll 1
    for (int pass = 0; pass < (G.T_flip ? 2 : 1); ++pass) {
        const float m = pass_mean(img, g, G, pass ? G.T : 0, c, y, pass ? G.W - 1 - x : x, pass ? k.cntf : k.cnt);
        s = pass ? 0.5f * (s + m) : m;
    }
    return s;
}

// G describes the scaled frame (G.H = Hs, G.W = Ws); (H, W) is the output
__global__ __launch_bounds__(kThreads) void accumulate_kernel(const float *tiles, TileGrid g, Geometry G, int H, int W,
                                                              const float *score_in, float *score_out, int divide_by,
                                                              const int64_t *labels, long long ignore, uint8_t *pred,
                                                              int64_t *conf) {
    EVAL_DYNAMIC_LDS(hist);
    const int C = G.C, n = blockIdx.y;
    const unsigned HW = (unsigned)(H * W);
    const int words = (C * C + 1) >> 1;
    if (conf) {
        for (int i = threadIdx.x; i < words; i += kThreads) hist[i] = 0u;
        __syncthreads();
    }
    const float *img = tiles + (size_t)n * (G.T + G.T_flip) * C * G.h * G.w;
    const unsigned base = blockIdx.x * (unsigned)kPixPerBlock + threadIdx.x;
    for (int k = 0; k < kPixPerThread; ++k) {
        const unsigned i = base + (unsigned)(k * kThreads);
        if (i >= HW) break;
        const int y = (int)(i / (unsigned)W), x = (int)(i - (unsigned)y * (unsigned)W);
        const Axis ay = axis_tap(y, G.H, H), ax = axis_tap(x, G.W, W);
        const bool two_y = ay.l != 0.f, two_x = ax.l != 0.f;
        // tap j of the pixel: bit 0 the second column, bit 1 the second row; its cover counts (<= 64) in byte j of cnt / cntf
        unsigned cnt = 0u, cntf = 0u;
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
            if (((j & 1) && !two_x) || ((j & 2) && !two_y)) continue;
            const Cover k = cover_counts(g, G, (j & 2) ? ay.i1 : ay.i0, (j & 1) ? ax.i1 : ax.i0);
            cnt |= (unsigned)k.cnt << (8 * j);
            cntf |= (unsigned)k.cntf << (8 * j);
        }
        float best = 0.f;
        int arg = 0;
        for (int c = 0; c < C; ++c) {
            float r = 0.f, v = 0.f;                   // the score at the pixel, the lerp along W of the current row
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                if (((j & 1) && !two_x) || ((j & 2) && !two_y)) continue;
                const Cover k = {(int)((cnt >> (8 * j)) & 0xffu), (int)((cntf >> (8 * j)) & 0xffu)};
                const float s = scaled_score(img, g, G, c, (j & 2) ? ay.i1 : ay.i0, (j & 1) ? ax.i1 : ax.i0, k);
                v = (j & 1) ? lerp(v, s, ax.l) : s;
                if ((j & 1) || !two_x) r = (j & 2) ? lerp(r, v, ay.l) : v;      // the row is complete
            }
            const size_t at = ((size_t)n * C + c) * HW + i;
            float s = score_in ? score_in[at] + r : r;
            if (divide_by > 0) s /= (float)divide_by;
            if (score_out) score_out[at] = s;
            if (first_maximum(c, s, best)) {          // as np.argmax: a NaN is one
                best = s;
                arg = c;
            }
        }
        if (pred) pred[(size_t)n * HW + i] = (uint8_t)arg;
        if (conf) {
            const long long lab = labels[(size_t)n * HW + i];
            if (lab != ignore && lab >= 0 && lab < C) {
                const int b = (int)lab * C + arg;
                lds_add(&hist[b >> 1], (b & 1) ? 0x10000u : 1u);
            }
        }
    }
    if (conf) {
        __syncthreads();
        for (int i = threadIdx.x; i < words; i += kThreads) {
            const unsigned v = hist[i];
            if (v & 0xffffu) global_add(conf + 2 * i, v & 0xffffu);
            if (v >> 16) global_add(conf + 2 * i + 1, v >> 16);
        }
    }
}

}  // namespace mseval
