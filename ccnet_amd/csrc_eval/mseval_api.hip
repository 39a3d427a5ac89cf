// mseval_api.hip -- the C ABI of include/ccnet_mseval.h (libccnet_mseval.so): argument checks and one launch per call.
// The second translation unit of the evaluation row: it shares eval_sample.hpp and eval_platform.hpp with eval_api.hip and
// nothing else.  Launches go on the caller's stream; the tile origins travel as a kernel argument; nothing waits for the device.
#include "ccnet_mseval.h"

#include "mseval_kernels.hpp"

#define CCNET_ERROR_PREFIX "ccnet_mseval: "
#include "../csrc_common/ccnet_host.hpp"

namespace {

// PyTorch's area_pixel_compute_scale for align_corners=True, in fp32
float align_corners_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// the checks both calls share on the tile grid of the scaled image; fills g
int read_grid(segeval::TileGrid &g, int T, int T_flip, const int *tile_y1x1, int tile_H, int tile_W, int Hs, int Ws) {
    if (T < 1 || T > segeval::kMaxTiles) return fail(-1, "T=%d outside [1, %d]", T, segeval::kMaxTiles);
    if (T_flip != 0 && T_flip != T) return fail(-1, "T_flip=%d is neither 0 nor T=%d", T_flip, T);
    if (tile_H < 1 || tile_W < 1 || Hs < 1 || Ws < 1) return fail(-1, "bad shape tile=%dx%d scaled=%dx%d", tile_H, tile_W, Hs, Ws);
    if ((long long)Hs * Ws > 0x7fffffffLL || (long long)tile_H * tile_W > 0x7fffffffLL)
        return fail(-1, "shape too large: scaled=%dx%d tile=%dx%d", Hs, Ws, tile_H, tile_W);
    if (!tile_y1x1) return fail(-2, "NULL tile_y1x1");
    for (int t = 0; t < T; ++t) {
        g.y1[t] = tile_y1x1[2 * t];
        g.x1[t] = tile_y1x1[2 * t + 1];
        if (g.y1[t] < 0 || g.y1[t] >= Hs || g.x1[t] < 0 || g.x1[t] >= Ws)
            return fail(-1, "tile %d origin (%d, %d) outside the %dx%d scaled image", t, g.y1[t], g.x1[t], Hs, Ws);
        if ((long long)g.y1[t] + tile_H > 0x7fffffffLL || (long long)g.x1[t] + tile_W > 0x7fffffffLL)
            return fail(-1, "shape too large: tile %d origin (%d, %d) + tile=%dx%d", t, g.y1[t], g.x1[t], tile_H, tile_W);
    }
    return 0;
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ccnet_mseval_version(void) { return CCNET_MSEVAL_VERSION; }
__attribute__((visibility("default"))) const char *ccnet_mseval_arch(void) { return "gfx950"; }
__attribute__((visibility("default"))) const char *ccnet_mseval_last_error_string(void) { return g_err; }

__attribute__((visibility("default"))) int ccnet_mseval_tiles_f32(const float *image, int N, int Cin, int H, int W, int Hs,
                                                                  int Ws, int T, int T_flip, const int *tile_y1x1, int tile_H,
                                                                  int tile_W, int first, int count, float *tiles_out,
                                                                  void *stream) {
    static_assert(CCNET_MSEVAL_MAX_TILES == segeval::kMaxTiles && CCNET_MSEVAL_MAX_CLASSES == segeval::kMaxClasses, "header");
    if (N < 1 || Cin < 1 || H < 1 || W < 1) return fail(-1, "bad shape N=%d Cin=%d image=%dx%d", N, Cin, H, W);
    if ((long long)H * W > 0x7fffffffLL || N > 65535) return fail(-1, "shape too large: N=%d image=%dx%d", N, H, W);
    segeval::TileGrid g = {};
    if (int rc = read_grid(g, T, T_flip, tile_y1x1, tile_H, tile_W, Hs, Ws)) return rc;
    if (first < 0 || count < 1 || first > T + T_flip - count)
        return fail(-1, "entries [%d, %d + %d) outside the %d tiles of an image", first, first, count, T + T_flip);
    if (!image || !tiles_out) return fail(-2, "NULL image or tiles_out");
    const mseval::TilesGeometry Q = {Cin, H, W, Hs, Ws, T, tile_H, tile_W, first, count};
    const dim3 grid((unsigned)(((long long)tile_H * tile_W + segeval::kThreads - 1) / segeval::kThreads), (unsigned)count,
                    (unsigned)N);
    EVAL_LAUNCH(mseval::tiles_kernel, grid, dim3(segeval::kThreads), 0, static_cast<hipStream_t>(stream), image, g, Q, tiles_out);
    return launched("tiles");
}

__attribute__((visibility("default"))) int ccnet_mseval_accumulate_f32(
    const float *tile_logits, int T, int T_flip, const int *tile_y1x1, int N, int C, int h, int w, int tile_H, int tile_W, int Hs,
    int Ws, int H, int W, const float *score_in, float *score_out, int divide_by, const int64_t *labels, long long ignore_label,
    uint8_t *pred_out, int64_t *confusion, void *stream) {
    if (C < 1 || C > segeval::kMaxClasses) return fail(-1, "C=%d outside [1, %d]", C, segeval::kMaxClasses);
    if (N < 1 || h < 1 || w < 1 || H < 1 || W < 1) return fail(-1, "bad shape N=%d h=%d w=%d image=%dx%d", N, h, w, H, W);
    if (divide_by < 0) return fail(-1, "divide_by=%d is negative", divide_by);
    segeval::TileGrid g = {};
    if (int rc = read_grid(g, T, T_flip, tile_y1x1, tile_H, tile_W, Hs, Ws)) return rc;
    if ((long long)H * W > 0x7fffffffLL || (long long)h * w > 0x7fffffffLL ||
        (long long)N * (T + T_flip) * C * ((long long)h * w) > (1LL << 40) || N > 65535)
        return fail(-1, "shape too large: N=%d image=%dx%d logits=%dx%d", N, H, W, h, w);
    if (!tile_logits) return fail(-2, "NULL tile_logits");
    if (confusion && !labels) return fail(-2, "confusion given without labels");
    const segeval::Geometry G = {T, T_flip, C, h, w, tile_H, tile_W, Hs, Ws, align_corners_scale(h, tile_H),
                                 align_corners_scale(w, tile_W)};
    const int lds = confusion ? segeval::hist_words(C) * 4 : 0;
    if (lds > 65536 && segeval::allow_dynamic_lds(reinterpret_cast<const void *>(&mseval::accumulate_kernel), lds))
        return fail(-4, "cannot grant %d bytes of LDS for C=%d", lds, C);
    const dim3 grid((unsigned)(((long long)H * W + segeval::kPixPerBlock - 1) / segeval::kPixPerBlock), (unsigned)N);
    EVAL_LAUNCH(mseval::accumulate_kernel, grid, dim3(segeval::kThreads), lds, static_cast<hipStream_t>(stream), tile_logits, g, G,
                H, W, score_in, score_out, divide_by, labels, ignore_label, pred_out, confusion);
    return launched("accumulate");
}

}  // extern "C"
