// ohem_api.hip -- the C ABI of include/ccnet_ohem.h (libccnet_ohem.so): argument checks, workspace layout, launches.
// Every launch goes on the caller's stream and nothing waits for the device.
#include "ccnet_ohem.h"

#include <math.h>

#include "ohem_kernels.hpp"

#define CCNET_ERROR_PREFIX "ccnet_ohem: "
#include "../csrc_common/ccnet_host.hpp"

namespace {

using ohem::zoom_len;      // (scipy.ndimage.zoom's output length and source step: ohem_kernels.hpp)
using ohem::zoom_step;

struct Layout {
    int N, ho, wo, M, nblk;
    size_t keys, part_sum, part_cnt, pix_lse, pix_tgt, scalars, total;
};

bool layout(int B, int C, int H, int W, int factor, Layout &L) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || factor < 1) return false;
    if ((long long)B * C * H * W > 0x7fffffffLL) return false;
    L.N = B * H * W;
    L.ho = zoom_len(H, factor);
    L.wo = zoom_len(W, factor);
    L.M = B * L.ho * L.wo;
    L.nblk = (L.N + ohem::kPixThreads - 1) / ohem::kPixThreads;
    size_t o = 0;
    L.keys = o;     o += align256(sizeof(uint32_t) * L.M);
    L.part_sum = o; o += align256(sizeof(float) * L.nblk);
    L.part_cnt = o; o += align256(sizeof(int) * L.nblk);
    L.pix_lse = o;  o += align256(sizeof(float) * L.N);
    L.pix_tgt = o;  o += align256(sizeof(int) * L.N);
    L.scalars = o;  o += align256(sizeof(ohem::Scalars));
    L.total = o;
    return true;
}

unsigned blocks(int n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ccnet_ohem_version(void) { return CCNET_OHEM_VERSION; }
__attribute__((visibility("default"))) const char *ccnet_ohem_arch(void) { return "gfx950"; }
__attribute__((visibility("default"))) const char *ccnet_ohem_last_error_string(void) { return g_err; }

__attribute__((visibility("default"))) size_t ccnet_ohem_workspace_bytes(int B, int C, int H, int W, int factor) {
    Layout L;
    return layout(B, C, H, W, factor, L) ? L.total : 0;
}

__attribute__((visibility("default"))) int ccnet_ohem_forward_f32(const float *logits, const int64_t *labels, float *loss,
                                                                  float *threshold, int *kept, int *num_valid, void *workspace,
                                                                  size_t workspace_bytes, int B, int C, int H, int W,
                                                                  long long ignore_label, float thresh, int min_kept,
                                                                  int factor, void *stream) {
    Layout L;
    if (!layout(B, C, H, W, factor, L))
        return fail(-1, "forward: bad shape B=%d C=%d H=%d W=%d factor=%d", B, C, H, W, factor);
    if (min_kept < 0 || !(thresh == thresh)) return fail(-1, "forward: bad min_kept=%d or thresh", min_kept);
    if (!logits || !labels || !loss || !workspace) return fail(-2, "forward: NULL logits, labels, loss or workspace");
    if (workspace_bytes < L.total) return fail(-3, "forward: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t *keys = at<uint32_t>(workspace, L.keys);
    ohem::Scalars *sc = at<ohem::Scalars>(workspace, L.scalars);
    if (L.M > 0)
        OHEM_LAUNCH(ohem::zoom_keys_kernel, dim3(blocks(L.M, ohem::kPixThreads)), dim3(ohem::kPixThreads), s, logits, labels,
                    keys, B, C, H, W, L.ho, L.wo, zoom_step(H, L.ho), zoom_step(W, L.wo), ignore_label);
    OHEM_LAUNCH(ohem::select_kernel, dim3(1), dim3(ohem::kSelectThreads), s, (const uint32_t *)keys, L.M,
                min_kept / (factor * factor), thresh, sc, threshold, num_valid);
    OHEM_LAUNCH(ohem::forward_kernel, dim3(L.nblk), dim3(ohem::kPixThreads), s, logits, labels, (const ohem::Scalars *)sc,
                at<float>(workspace, L.part_sum), at<int>(workspace, L.part_cnt), at<float>(workspace, L.pix_lse),
                at<int>(workspace, L.pix_tgt), C, H * W, L.N, ignore_label);
    OHEM_LAUNCH(ohem::finalize_kernel, dim3(1), dim3(ohem::kFinalThreads), s, (const float *)at<float>(workspace, L.part_sum),
                (const int *)at<int>(workspace, L.part_cnt), L.nblk, sc, loss, kept);
    return launched("forward");
}

__attribute__((visibility("default"))) int ccnet_ohem_backward_f32(const float *grad_out, const float *logits, float *grad_logits,
                                                                   const void *workspace, size_t workspace_bytes, int B, int C,
                                                                   int H, int W, int factor, void *stream) {
    Layout L;
    if (!layout(B, C, H, W, factor, L))
        return fail(-1, "backward: bad shape B=%d C=%d H=%d W=%d factor=%d", B, C, H, W, factor);
    if (!grad_out || !logits || !grad_logits || !workspace)
        return fail(-2, "backward: NULL grad_out, logits, grad_logits or workspace");
    if (workspace_bytes < L.total) return fail(-3, "backward: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    void *ws = const_cast<void *>(workspace);
    OHEM_LAUNCH(ohem::backward_kernel, dim3(L.nblk), dim3(ohem::kPixThreads), static_cast<hipStream_t>(stream), grad_out, logits,
                grad_logits, (const float *)at<float>(ws, L.pix_lse), (const int *)at<int>(ws, L.pix_tgt),
                (const ohem::Scalars *)at<ohem::Scalars>(ws, L.scalars), C, H * W, L.N);
    return launched("backward");
}

}  // extern "C"
