// celovasz_api.hip -- the C ABI of include/ccnet_celovasz.h (libccnet_celovasz.so): argument checks, workspace layout, launches.
// Every launch goes on the caller's stream and nothing waits for the device.
#include "ccnet_celovasz.h"

#include "celovasz_kernels.hpp"

#define CCNET_ERROR_PREFIX "ccnet_celovasz: "
#include "../csrc_common/ccnet_host.hpp"

#include "lovasz_launch.hpp"

namespace {

constexpr int kMaxSide = 1 << 20;      // fp32 source coordinates stay exact integers' neighbours well below 2^24 (ccnet_dsn.h)

struct Layout {
    int N, nblk;
    float sh, sw;
    size_t pix_lse, pix_tgt, pix_dot, part_sum, part_cnt, scalars, sort, total;
    lovasz::Layout S;                  // the Lovász workspace, at offset `sort`
};

// PyTorch's area_pixel_compute_scale for align_corners=True, in fp32
float axis_scale(int n_in, int n_out) { return n_out > 1 ? (float)(n_in - 1) / (n_out - 1) : 0.f; }

// the intersection of ccnet_dsn.h's shapes and ccnet_lovasz.h's
bool layout(int B, int C, int h, int w, int H, int W, int per_image, Layout &L) {
    if (B < 1 || B > 32767 || h < 1 || w < 1 || H < h || W < w || H > kMaxSide || W > kMaxSide) return false;
    if ((long long)B * H * W > 0x7fffffffLL || (long long)B * C * h * w > 0x7fffffffLL) return false;
    if (!lovasz::layout(B, C, H, W, per_image, L.S)) return false;
    L.N = B * H * W;
    L.nblk = (L.N + celovasz::kPixThreads - 1) / celovasz::kPixThreads;
    L.sh = axis_scale(h, H);
    L.sw = axis_scale(w, W);
    size_t o = 0;
    L.pix_lse = o;  o += align256(sizeof(float) * L.N);
    L.pix_tgt = o;  o += align256(sizeof(int16_t) * L.N);
    L.pix_dot = o;  o += align256(sizeof(float) * L.N);
    L.part_sum = o; o += align256(sizeof(float) * L.nblk);
    L.part_cnt = o; o += align256(sizeof(int) * 2 * L.nblk);
    L.scalars = o;  o += align256(sizeof(celovasz::Scalars));
    L.sort = o;     o += L.S.total;
    L.total = o;
    return true;
}

unsigned blocks(int n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ccnet_celovasz_version(void) { return CCNET_CELOVASZ_VERSION; }
__attribute__((visibility("default"))) const char *ccnet_celovasz_arch(void) { return "gfx950"; }
__attribute__((visibility("default"))) const char *ccnet_celovasz_last_error(void) { return g_err; }

__attribute__((visibility("default"))) size_t ccnet_celovasz_workspace_bytes(int B, int C, int h, int w, int H, int W,
                                                                             int per_image) {
    Layout L;
    return layout(B, C, h, w, H, W, per_image, L) ? L.total : 0;
}

__attribute__((visibility("default"))) int ccnet_celovasz_forward_f32(const float *logits, const int64_t *target,
                                                                      long long ignore_index, int per_image, int present_only,
                                                                      const unsigned char *class_weights, float *loss,
                                                                      float *head_loss, int *counts, void *workspace,
                                                                      size_t workspace_bytes, int B, int C, int h, int w, int H,
                                                                      int W, void *stream) {
    Layout L;
    if (!layout(B, C, h, w, H, W, per_image, L))
        return fail(-1, "forward: unsupported shape B=%d C=%d h=%d w=%d H=%d W=%d per_image=%d (2 <= C <= 256, h <= H, w <= W, "
                        "at most 2^24 pixels a segment)", B, C, h, w, H, W, per_image);
    if (!logits || !target || !loss || !workspace) return fail(-2, "forward: NULL logits, target, loss or workspace");
    if (workspace_bytes < L.total) return fail(-3, "forward: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    const lovasz::ClassSel sel = lovasz::class_sel(class_weights, C, present_only);
    hipStream_t s = static_cast<hipStream_t>(stream);
    void *ws = workspace, *sort = at<char>(ws, L.sort);
    celovasz::Scalars *sc = at<celovasz::Scalars>(ws, L.scalars);
    float *part_sum = at<float>(ws, L.part_sum);
    int *part_cnt = at<int>(ws, L.part_cnt);
    const dim3 block(celovasz::kPixThreads);
    LOVASZ_LAUNCH(celovasz::pixel_errors_kernel, dim3((unsigned)L.nblk), block, s, logits, target,
                  at<uint32_t>(sort, L.S.keys[0]), at<uint32_t>(sort, L.S.pays[0]), part_sum, part_cnt, at<float>(ws, L.pix_lse),
                  at<int16_t>(ws, L.pix_tgt), C, h, w, H, W, L.N, L.S.L, per_image ? 1 : 0, L.sh, L.sw, ignore_index);
    lovasz::sort_scan_finalize(sort, L.S, B, C, per_image, sel, &sc->ls, &sc->n_kept, s);
    LOVASZ_LAUNCH(celovasz::finalize_kernel, dim3(1), dim3(celovasz::kFinalThreads), s, (const float *)part_sum,
                  (const int *)part_cnt, L.nblk, sc, loss, head_loss, counts);
    LOVASZ_LAUNCH(celovasz::pixel_dot_kernel, dim3(blocks(L.S.HW, celovasz::kPixThreads), (unsigned)B), block, s, logits,
                  (const float *)at<float>(sort, L.S.g), (const int *)at<int>(sort, L.S.seg_mult),
                  (const int *)at<int>(sort, L.S.seg_den), (const float *)at<float>(ws, L.pix_lse),
                  (const int16_t *)at<int16_t>(ws, L.pix_tgt), at<float>(ws, L.pix_dot), B, C, h, w, H, W, L.S.L,
                  per_image ? 1 : 0, L.sh, L.sw);
    return launched("forward");
}

__attribute__((visibility("default"))) int ccnet_celovasz_backward_f32(const float *grad_out, const float *logits, float *grad,
                                                                       const void *workspace, size_t workspace_bytes, int B,
                                                                       int C, int h, int w, int H, int W, int per_image,
                                                                       void *stream) {
    Layout L;
    if (!layout(B, C, h, w, H, W, per_image, L))
        return fail(-1, "backward: unsupported shape B=%d C=%d h=%d w=%d H=%d W=%d per_image=%d", B, C, h, w, H, W, per_image);
    if (!grad_out || !logits || !grad || !workspace) return fail(-2, "backward: NULL grad_out, logits, grad or workspace");
    if (workspace_bytes < L.total) return fail(-3, "backward: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    void *ws = const_cast<void *>(workspace), *sort = at<char>(ws, L.sort);
    const dim3 grid(blocks(h * w, celovasz::kPixThreads), (unsigned)C, (unsigned)B);
    LOVASZ_LAUNCH(celovasz::backward_kernel, grid, dim3(celovasz::kPixThreads), static_cast<hipStream_t>(stream), grad_out,
                  logits, grad, (const float *)at<float>(sort, L.S.g), (const int *)at<int>(sort, L.S.seg_mult),
                  (const int *)at<int>(sort, L.S.seg_den), (const float *)at<float>(ws, L.pix_lse),
                  (const int16_t *)at<int16_t>(ws, L.pix_tgt), (const float *)at<float>(ws, L.pix_dot),
                  (const celovasz::Scalars *)at<celovasz::Scalars>(ws, L.scalars), B, C, h, w, H, W, L.S.L, per_image ? 1 : 0,
                  L.sh, L.sw);
    return launched("backward");
}

}  // extern "C"
