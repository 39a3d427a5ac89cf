// eval_kernels.hpp -- the one kernel behind include/ccnet_eval.h.
//
//   sliding   grid (pixel blocks, N), 256 threads, 4096 pixels a workgroup (16 a thread, consecutive threads on consecutive
//             pixels of a row: every load of labels and every store of pred / probs is coalesced along W).  Per pixel and
//             class it samples the covering tiles' 1/8-resolution logits bilinearly (PyTorch's align_corners=True
//             arithmetic), averages them per pass, averages the passes, writes the optional score and keeps the first
//             maximum; then it counts (label, pred) in a workgroup-private LDS histogram.  The 8x up-sampled tiles and the
//             full-resolution score map are never materialised unless probs is asked for: the 64 output pixels that share
//             one 2 x 2 footprint read it from L1 / L2.
//
// The histogram holds the whole C x C matrix as 16-bit counters, two to an LDS word (a workgroup counts at most 4096 pixels,
// so a counter never carries into its neighbour): C * C * 2 bytes of dynamic LDS, 724 B at C = 19, 45 000 B at C = 150,
// 128 KiB at C = 256.  Only workgroups that count allocate it.  After the pixels, each nonzero counter is added to the int64
// confusion matrix with one integer atomic: the counts are exact and independent of the order of arrival.
#pragma once
#include <eval_platform.hpp>

#include <stddef.h>
#include <stdint.h>

namespace segeval {

constexpr int kThreads = 256;
constexpr int kPixPerThread = 16;
constexpr int kPixPerBlock = kThreads * kPixPerThread;   // < 65536: the 16-bit counters cannot overflow
constexpr int kMaxTiles = 64;
constexpr int kMaxClasses = 256;

struct TileGrid {                  // the tiles' top-left corners, passed by value as a kernel argument
    int y1[kMaxTiles];
    int x1[kMaxTiles];
};

struct Geometry {
    int T, T_flip, C, h, w, tile_H, tile_W, H, W;
    float sy, sx;                  // area_pixel_compute_scale: (float)(h - 1) / (tile_H - 1), 0 for a one-pixel tile
};

inline int hist_words(int C) { return (C * C + 1) / 2; }

__device__ __forceinline__ bool covers(const TileGrid &g, const Geometry &G, int t, int y, int x) {
    const int y1 = g.y1[t], x1 = g.x1[t];
    return y >= y1 && y < y1 + G.tile_H && x >= x1 && x < x1 + G.tile_W;    // (y, x) is inside the image already
}

// upsample_bilinear2d, align_corners=True, at tile-local (ly, lx) of one (h, w) logit plane
__device__ __forceinline__ float sample(const float *plane, const Geometry &G, int ly, int lx) {
    const float ry = G.sy * (float)ly, rx = G.sx * (float)lx;
    const int y0 = (int)ry, x0 = (int)rx;
    const int yp = y0 < G.h - 1 ? G.w : 0, xp = x0 < G.w - 1 ? 1 : 0;
    const float y1l = ry - (float)y0, x1l = rx - (float)x0;
    const float y0l = 1.f - y1l, x0l = 1.f - x1l;
    const float *p = plane + (size_t)y0 * G.w + x0;
    return y0l * (x0l * p[0] + x1l * p[xp]) + y1l * (x0l * p[yp] + x1l * p[yp + xp]);
}

// mean over the tiles of one pass (tiles [first, first + T) of the image) that cover (y, x)
__device__ __forceinline__ float pass_mean(const float *img, const TileGrid &g, const Geometry &G, int first, int c, int y,
                                           int x, int count) {
    const size_t plane = (size_t)G.h * G.w;
    float s = 0.f;
    for (int t = 0; t < G.T; ++t)
        if (covers(g, G, t, y, x)) s += sample(img + ((size_t)(first + t) * G.C + c) * plane, G, y - g.y1[t], x - g.x1[t]);
    return s / (float)count;
}

__global__ __launch_bounds__(kThreads) void sliding_kernel(const float *tiles, TileGrid g, Geometry G, const int64_t *labels,
                                                           long long ignore, float *probs, uint8_t *pred, int64_t *conf) {
    EVAL_DYNAMIC_LDS(hist);
    const int C = G.C, HW = G.H * G.W, n = blockIdx.y;
    const int words = (C * C + 1) >> 1;
    if (conf) {
        for (int i = threadIdx.x; i < words; i += kThreads) hist[i] = 0u;
        __syncthreads();
    }
    const float *img = tiles + (size_t)n * (G.T + G.T_flip) * C * G.h * G.w;
    const int base = blockIdx.x * kPixPerBlock + threadIdx.x;
    for (int k = 0; k < kPixPerThread; ++k) {
        const int i = base + k * kThreads;
        if (i >= HW) break;
        const int y = i / G.W, x = i - y * G.W, xf = G.W - 1 - x;
        int cnt = 0, cntf = 0;
        for (int t = 0; t < G.T; ++t) {
            cnt += covers(g, G, t, y, x);
            cntf += covers(g, G, t, y, xf);
        }
        float best = 0.f;
        int arg = 0;
        for (int c = 0; c < C; ++c) {
            float s = pass_mean(img, g, G, 0, c, y, x, cnt);
            if (G.T_flip) s = 0.5f * (s + pass_mean(img, g, G, G.T, c, y, xf, cntf));
            if (probs) probs[((size_t)n * C + c) * HW + i] = s;
            if (c == 0 || s > best) {                 // the first maximum, as np.argmax
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

}  // namespace segeval
