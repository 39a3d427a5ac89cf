// eval_api.hip -- the C ABI of include/ccnet_eval.h (libccnet_eval.so): argument checks and the one launch.
// The launch goes on the caller's stream; the tile origins travel as a kernel argument and nothing waits for the device.
#include "ccnet_eval.h"

#include "eval_kernels.hpp"

#define CCNET_ERROR_PREFIX "ccnet_eval: "
#include "../csrc_common/ccnet_host.hpp"

namespace {

// PyTorch's area_pixel_compute_scale for align_corners=True, in fp32
float align_corners_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ccnet_eval_version(void) { return CCNET_EVAL_VERSION; }
__attribute__((visibility("default"))) const char *ccnet_eval_arch(void) { return "gfx950"; }
__attribute__((visibility("default"))) const char *ccnet_eval_last_error_string(void) { return g_err; }

__attribute__((visibility("default"))) int ccnet_eval_sliding_f32(const float *tile_logits, int T, int T_flip,
                                                                  const int *tile_y1x1, int N, int C, int h, int w,
                                                                  int tile_H, int tile_W, int H, int W, const int64_t *labels,
                                                                  long long ignore_label, float *probs_out, uint8_t *pred_out,
                                                                  int64_t *confusion, void *stream) {
    static_assert(CCNET_EVAL_MAX_TILES == segeval::kMaxTiles && CCNET_EVAL_MAX_CLASSES == segeval::kMaxClasses, "header");
    if (C < 1 || C > segeval::kMaxClasses) return fail(-1, "C=%d outside [1, %d]", C, segeval::kMaxClasses);
    if (T < 1 || T > segeval::kMaxTiles) return fail(-1, "T=%d outside [1, %d]", T, segeval::kMaxTiles);
    if (T_flip != 0 && T_flip != T) return fail(-1, "T_flip=%d is neither 0 nor T=%d", T_flip, T);
    if (N < 1 || h < 1 || w < 1 || tile_H < 1 || tile_W < 1 || H < 1 || W < 1)
        return fail(-1, "bad shape N=%d h=%d w=%d tile=%dx%d image=%dx%d", N, h, w, tile_H, tile_W, H, W);
    if ((long long)H * W > 0x7fffffffLL || (long long)N * (T + T_flip) * C * h * w > (1LL << 40) || N > 65535)
        return fail(-1, "shape too large: N=%d image=%dx%d", N, H, W);
    if (!tile_logits || !tile_y1x1) return fail(-2, "NULL tile_logits or tile_y1x1");
    if (confusion && !labels) return fail(-2, "confusion given without labels");
    segeval::TileGrid g = {};
    for (int t = 0; t < T; ++t) {
        g.y1[t] = tile_y1x1[2 * t];
        g.x1[t] = tile_y1x1[2 * t + 1];
        if (g.y1[t] < 0 || g.y1[t] >= H || g.x1[t] < 0 || g.x1[t] >= W)
            return fail(-1, "tile %d origin (%d, %d) outside the %dx%d image", t, g.y1[t], g.x1[t], H, W);
    }
    segeval::Geometry G = {T, T_flip, C, h, w, tile_H, tile_W, H, W, align_corners_scale(h, tile_H),
                           align_corners_scale(w, tile_W)};
    const int lds = confusion ? segeval::hist_words(C) * 4 : 0;
    if (lds > 65536 && segeval::allow_dynamic_lds(reinterpret_cast<const void *>(&segeval::sliding_kernel), lds))
        return fail(-4, "cannot grant %d bytes of LDS for C=%d", lds, C);
    const dim3 grid((unsigned)((H * W + segeval::kPixPerBlock - 1) / segeval::kPixPerBlock), (unsigned)N);
    EVAL_LAUNCH(segeval::sliding_kernel, grid, dim3(segeval::kThreads), lds, static_cast<hipStream_t>(stream), tile_logits, g, G,
                labels, ignore_label, probs_out, pred_out, confusion);
    return launched("sliding");
}

}  // extern "C"
