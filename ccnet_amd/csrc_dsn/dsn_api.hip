// dsn_api.hip -- the C ABI of include/ccnet_dsn.h (libccnet_dsn.so): argument checks, workspace layout, launches.
// Every launch goes on the caller's stream and nothing waits for the device.
#include "ccnet_dsn.h"

#include "dsn_kernels.hpp"

#define CCNET_ERROR_PREFIX "ccnet_dsn: "
#include "../csrc_common/ccnet_host.hpp"

namespace {

constexpr int kMaxSide = 1 << 20;      // fp32 source coordinates stay exact integers' neighbours well below 2^24

struct Layout {
    int N, nblk;
    float sh, sw;
    size_t pix_lse, pix_tgt, part_sum, part_cnt, scalars, total;
};

// PyTorch's area_pixel_compute_scale for align_corners=True, in fp32
float axis_scale(int n_in, int n_out) { return n_out > 1 ? (float)(n_in - 1) / (n_out - 1) : 0.f; }

bool layout(int B, int C, int h, int w, int H, int W, int heads, Layout &L) {
    if (B < 1 || B > 32767 || C < 1 || C > dsn::kMaxClasses || h < 1 || w < 1 || H < h || W < w) return false;
    if (H > kMaxSide || W > kMaxSide || (heads != 1 && heads != 2)) return false;
    if ((long long)B * H * W > 0x7fffffffLL || (long long)B * C * h * w > 0x7fffffffLL) return false;
    L.N = B * H * W;
    L.nblk = (L.N + dsn::kPixThreads - 1) / dsn::kPixThreads;
    L.sh = axis_scale(h, H);
    L.sw = axis_scale(w, W);
    size_t o = 0;
    L.pix_lse = o;  o += align256(sizeof(float) * L.N * heads);
    L.pix_tgt = o;  o += align256(sizeof(int16_t) * L.N);
    L.part_sum = o; o += align256(sizeof(float) * 2 * L.nblk);
    L.part_cnt = o; o += align256(sizeof(int) * 2 * L.nblk);
    L.scalars = o;  o += align256(sizeof(dsn::Scalars));
    L.total = o;
    return true;
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ccnet_dsn_version(void) { return CCNET_DSN_VERSION; }
__attribute__((visibility("default"))) const char *ccnet_dsn_arch(void) { return "gfx950"; }
__attribute__((visibility("default"))) const char *ccnet_dsn_last_error_string(void) { return g_err; }

__attribute__((visibility("default"))) size_t ccnet_dsn_workspace_bytes(int B, int C, int h, int w, int H, int W, int heads) {
    Layout L;
    return layout(B, C, h, w, H, W, heads, L) ? L.total : 0;
}

__attribute__((visibility("default"))) int ccnet_dsn_forward_f32(const float *logits0, const float *logits1, const int64_t *target,
                                                                 float weight0, float weight1, float *loss, float *head_loss,
                                                                 int *counts, void *workspace, size_t workspace_bytes, int B,
                                                                 int C, int h, int w, int H, int W, int heads,
                                                                 long long ignore_index, void *stream) {
    Layout L;
    if (!layout(B, C, h, w, H, W, heads, L))
        return fail(-1, "forward: unsupported shape B=%d C=%d h=%d w=%d H=%d W=%d heads=%d", B, C, h, w, H, W, heads);
    if (!logits0 || (heads == 2 && !logits1) || !target || !loss || !workspace)
        return fail(-2, "forward: NULL logits, target, loss or workspace");
    if (workspace_bytes < L.total) return fail(-3, "forward: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *part_sum = at<float>(workspace, L.part_sum);
    int *part_cnt = at<int>(workspace, L.part_cnt);
    DSN_LAUNCH(dsn::forward_kernel, dim3(L.nblk), dim3(dsn::kPixThreads), s, logits0, logits1, target, part_sum, part_cnt,
               at<float>(workspace, L.pix_lse), at<int16_t>(workspace, L.pix_tgt), C, h, w, H, W, L.N, heads, L.sh, L.sw,
               ignore_index);
    DSN_LAUNCH(dsn::finalize_kernel, dim3(1), dim3(dsn::kFinalThreads), s, (const float *)part_sum, (const int *)part_cnt, L.nblk,
               heads, weight0, weight1, at<dsn::Scalars>(workspace, L.scalars), loss, head_loss, counts);
    return launched("forward");
}

__attribute__((visibility("default"))) int ccnet_dsn_backward_f32(const float *grad_out, const float *logits0, const float *logits1,
                                                                  float *grad0, float *grad1, float weight0, float weight1,
                                                                  const void *workspace, size_t workspace_bytes, int B, int C,
                                                                  int h, int w, int H, int W, int heads, void *stream) {
    Layout L;
    if (!layout(B, C, h, w, H, W, heads, L))
        return fail(-1, "backward: unsupported shape B=%d C=%d h=%d w=%d H=%d W=%d heads=%d", B, C, h, w, H, W, heads);
    if (!grad_out || !logits0 || !grad0 || (heads == 2 && (!logits1 || !grad1)) || !workspace)
        return fail(-2, "backward: NULL grad_out, logits, grad or workspace");
    if (workspace_bytes < L.total) return fail(-3, "backward: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    void *ws = const_cast<void *>(workspace);
    const dim3 grid((unsigned)((h * w + dsn::kPixThreads - 1) / dsn::kPixThreads), (unsigned)C, (unsigned)(B * heads));
    DSN_LAUNCH(dsn::backward_kernel, grid, dim3(dsn::kPixThreads), static_cast<hipStream_t>(stream), grad_out, logits0, logits1,
               grad0, grad1, weight0, weight1, (const float *)at<float>(ws, L.pix_lse), (const int16_t *)at<int16_t>(ws, L.pix_tgt),
               (const dsn::Scalars *)at<dsn::Scalars>(ws, L.scalars), C, h, w, H, W, L.N, heads, L.sh, L.sw);
    return launched("backward");
}

}  // extern "C"
