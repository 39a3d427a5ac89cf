// ohemdsn_api.hip -- the C ABI of include/ccnet_ohemdsn.h (libccnet_ohemdsn.so): argument checks, workspace layout, launches.
// Every launch goes on the caller's stream and nothing waits for the device.
#include "ccnet_ohemdsn.h"

#include "ohemdsn_kernels.hpp"

#define CCNET_ERROR_PREFIX "ccnet_ohemdsn: "
#include "../csrc_common/ccnet_host.hpp"

namespace {

constexpr int kMaxSide = 1 << 20;      // fp32 source coordinates stay exact integers' neighbours well below 2^24

struct Layout {
    int N, ho, wo, M, nblk;
    float sh, sw;
    size_t keys, pix_lse, pix_tgt, part_sum, part_cnt, select, scalars, total;
};

// PyTorch's area_pixel_compute_scale for align_corners=True, in fp32
float axis_scale(int n_in, int n_out) { return n_out > 1 ? (float)(n_in - 1) / (n_out - 1) : 0.f; }

bool layout(int B, int C, int h, int w, int H, int W, int heads, int factor, Layout &L) {
    if (B < 1 || B > 32767 || C < 1 || C > dsn::kMaxClasses || h < 1 || w < 1 || H < h || W < w) return false;
    if (H > kMaxSide || W > kMaxSide || (heads != 1 && heads != 2) || factor < 1) return false;
    if ((long long)B * H * W > 0x7fffffffLL || (long long)B * C * h * w > 0x7fffffffLL) return false;
    L.N = B * H * W;
    L.ho = ohem::zoom_len(H, factor);
    L.wo = ohem::zoom_len(W, factor);
    L.M = B * L.ho * L.wo;
    L.nblk = (L.N + ohemdsn::kPixThreads - 1) / ohemdsn::kPixThreads;
    L.sh = axis_scale(h, H);
    L.sw = axis_scale(w, W);
    size_t o = 0;
    L.keys = o;     o += align256(sizeof(uint32_t) * L.M);
    L.pix_lse = o;  o += align256(sizeof(float) * L.N * heads);
    L.pix_tgt = o;  o += align256(sizeof(int16_t) * L.N);
    L.part_sum = o; o += align256(sizeof(float) * 2 * L.nblk);
    L.part_cnt = o; o += align256(sizeof(int) * 3 * L.nblk);
    L.select = o;   o += align256(sizeof(ohem::Scalars));
    L.scalars = o;  o += align256(sizeof(ohemdsn::Scalars));
    L.total = o;
    return true;
}

unsigned blocks(int n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ccnet_ohemdsn_version(void) { return CCNET_OHEMDSN_VERSION; }
__attribute__((visibility("default"))) const char *ccnet_ohemdsn_arch(void) { return "gfx950"; }
__attribute__((visibility("default"))) const char *ccnet_ohemdsn_last_error(void) { return g_err; }

__attribute__((visibility("default"))) size_t ccnet_ohemdsn_workspace_bytes(int B, int C, int h, int w, int H, int W, int heads,
                                                                            int factor) {
    Layout L;
    return layout(B, C, h, w, H, W, heads, factor, L) ? L.total : 0;
}

__attribute__((visibility("default"))) int ccnet_ohemdsn_forward_f32(const float *logits0, const float *logits1,
                                                                     const int64_t *target, long long ignore_index, float thresh,
                                                                     int min_kept, int factor, float *loss, float *head_loss,
                                                                     float *threshold, int *counts, void *workspace,
                                                                     size_t workspace_bytes, int B, int C, int h, int w, int H,
                                                                     int W, int heads, void *stream) {
    Layout L;
    if (!layout(B, C, h, w, H, W, heads, factor, L))
        return fail(-1, "forward: unsupported shape B=%d C=%d h=%d w=%d H=%d W=%d heads=%d factor=%d", B, C, h, w, H, W, heads,
                    factor);
    if (min_kept < 0 || !(thresh == thresh)) return fail(-1, "forward: bad min_kept=%d or thresh", min_kept);
    if (!logits0 || (heads == 2 && !logits1) || !target || !loss || !workspace)
        return fail(-2, "forward: NULL logits, target, loss or workspace");
    if (workspace_bytes < L.total) return fail(-3, "forward: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t *keys = at<uint32_t>(workspace, L.keys);
    ohem::Scalars *sel = at<ohem::Scalars>(workspace, L.select);
    float *part_sum = at<float>(workspace, L.part_sum);
    int *part_cnt = at<int>(workspace, L.part_cnt);
    if (L.M > 0)
        OHEM_LAUNCH(ohemdsn::zoom_keys_kernel, dim3(blocks(L.M, ohemdsn::kPixThreads)), dim3(ohemdsn::kPixThreads), s, logits0,
                    target, keys, B, C, h, w, H, W, L.ho, L.wo, ohem::zoom_step(H, L.ho), ohem::zoom_step(W, L.wo), L.sh, L.sw,
                    ignore_index);
    OHEM_LAUNCH(ohem::select_kernel, dim3(1), dim3(ohem::kSelectThreads), s, (const uint32_t *)keys, L.M,
                (int)(min_kept / ((long long)factor * factor)), thresh, sel, threshold, (int *)nullptr);
    OHEM_LAUNCH(ohemdsn::forward_kernel, dim3(L.nblk), dim3(ohemdsn::kPixThreads), s, logits0, logits1, target,
                (const ohem::Scalars *)sel, part_sum, part_cnt, at<float>(workspace, L.pix_lse),
                at<int16_t>(workspace, L.pix_tgt), C, h, w, H, W, L.N, heads, L.sh, L.sw, ignore_index);
    OHEM_LAUNCH(ohemdsn::finalize_kernel, dim3(1), dim3(ohemdsn::kFinalThreads), s, (const float *)part_sum,
                (const int *)part_cnt, L.nblk, heads, (const ohem::Scalars *)sel, at<ohemdsn::Scalars>(workspace, L.scalars), loss,
                head_loss, counts);
    return launched("forward");
}

__attribute__((visibility("default"))) int ccnet_ohemdsn_backward_f32(const float *grad_out, const float *logits0,
                                                                      const float *logits1, float *grad0, float *grad1,
                                                                      const void *workspace, size_t workspace_bytes, int B,
                                                                      int C, int h, int w, int H, int W, int heads, int factor,
                                                                      void *stream) {
    Layout L;
    if (!layout(B, C, h, w, H, W, heads, factor, L))
        return fail(-1, "backward: unsupported shape B=%d C=%d h=%d w=%d H=%d W=%d heads=%d factor=%d", B, C, h, w, H, W, heads,
                    factor);
    if (!grad_out || !logits0 || !grad0 || (heads == 2 && (!logits1 || !grad1)) || !workspace)
        return fail(-2, "backward: NULL grad_out, logits, grad or workspace");
    if (workspace_bytes < L.total) return fail(-3, "backward: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    void *ws = const_cast<void *>(workspace);
    const dim3 grid(blocks(h * w, ohemdsn::kPixThreads), (unsigned)C, (unsigned)(B * heads));
    OHEM_LAUNCH(ohemdsn::backward_kernel, grid, dim3(ohemdsn::kPixThreads), static_cast<hipStream_t>(stream), grad_out, logits0,
                logits1, grad0, grad1, (const float *)at<float>(ws, L.pix_lse), (const int16_t *)at<int16_t>(ws, L.pix_tgt),
                (const ohemdsn::Scalars *)at<ohemdsn::Scalars>(ws, L.scalars), C, h, w, H, W, L.N, heads, L.sh, L.sw);
    return launched("backward");
}

}  // extern "C"
