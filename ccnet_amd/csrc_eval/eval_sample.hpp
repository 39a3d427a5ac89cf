// eval_sample.hpp -- the per-tile sampling arithmetic that both translation units of the evaluation row use: the tile grid
// and geometry that travel as kernel arguments, the cover test, the bilinear sample of one tile's logits and the mean over
// one pass.  eval_kernels.hpp (libccnet_eval.so) and mseval_kernels.hpp (libccnet_mseval.so) include it, so the per-scale
// score of the multi-scale path is the single-scale score bit for bit.
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
//
// The compiler may not contract here, and the three fused multiply-adds are written out: which product of a * b + c * d it
// would fuse depends on the code around the inlined call, and sliding_kernel and accumulate_kernel then round differently
// (seen on gfx950 at small overlapping tiles: a tenth of the two libraries' scores one ulp apart at Hs == H, Ws == W, which
// mseval_kernels.hpp promises to be the same bits).  Unfused, lambda1 = source - index0 is also the header's.
__device__ __forceinline__ float sample(const float *plane, const Geometry &G, int ly, int lx) {
#pragma clang fp contract(off)
    const float ry = G.sy * (float)ly, rx = G.sx * (float)lx;
    const int y0 = (int)ry, x0 = (int)rx;
    const int yp = y0 < G.h - 1 ? G.w : 0, xp = x0 < G.w - 1 ? 1 : 0;
    const float y1l = ry - (float)y0, x1l = rx - (float)x0;
    const float y0l = 1.f - y1l, x0l = 1.f - x1l;
    const float *p = plane + (size_t)y0 * G.w + x0;
    const float top = __builtin_fmaf(x0l, p[0], x1l * p[xp]), bot = __builtin_fmaf(x0l, p[yp], x1l * p[yp + xp]);
    return __builtin_fmaf(y0l, top, y1l * bot);
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

// whether score s of class c replaces the best of classes [0, c): the first maximum, as np.argmax -- among equal scores the
// lowest class, and a NaN counts as the maximum (the first NaN wins).  Both kernels of the row take their prediction from here.
__device__ __forceinline__ bool first_maximum(int c, float s, float best) {
    return c == 0 || s > best || (s != s && best == best);
}

}  // namespace segeval
