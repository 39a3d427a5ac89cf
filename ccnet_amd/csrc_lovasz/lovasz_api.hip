// lovasz_api.hip -- the C ABI of include/ccnet_lovasz.h (libccnet_lovasz.so): argument checks, workspace layout, launches.
// Every launch goes on the caller's stream and nothing waits for the device.
#include "ccnet_lovasz.h"

#include "lovasz_kernels.hpp"

#define CCNET_ERROR_PREFIX "ccnet_lovasz: "
#include "../csrc_common/ccnet_host.hpp"

#include "lovasz_launch.hpp"

using lovasz::Layout;
using lovasz::layout;

extern "C" {

__attribute__((visibility("default"))) int ccnet_lovasz_version(void) { return CCNET_LOVASZ_VERSION; }
__attribute__((visibility("default"))) const char *ccnet_lovasz_arch(void) { return "gfx950"; }
__attribute__((visibility("default"))) const char *ccnet_lovasz_last_error_string(void) { return g_err; }

__attribute__((visibility("default"))) size_t ccnet_lovasz_workspace_bytes(int B, int C, int H, int W, int per_image) {
    Layout L;
    return layout(B, C, H, W, per_image, L) ? L.total : 0;
}

__attribute__((visibility("default"))) int ccnet_lovasz_forward_f32(const float *probas, const int64_t *labels, float *loss,
                                                                    int *n_kept, void *workspace, size_t workspace_bytes,
                                                                    int B, int C, int H, int W, long long ignore,
                                                                    int ignore_none, int per_image, int present_only,
                                                                    const unsigned char *class_weights, void *stream) {
    Layout L;
    if (!layout(B, C, H, W, per_image, L))
        return fail(-1, "forward: bad shape B=%d C=%d H=%d W=%d per_image=%d (2 <= C <= 256, at most 2^24 pixels a segment)",
                    B, C, H, W, per_image);
    if (!probas || !labels || !loss || !workspace) return fail(-2, "forward: NULL probas, labels, loss or workspace");
    if (workspace_bytes < L.total) return fail(-3, "forward: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    const lovasz::ClassSel sel = lovasz::class_sel(class_weights, C, present_only);
    hipStream_t s = static_cast<hipStream_t>(stream);
    void *ws = workspace;
    const dim3 pix((unsigned)((L.HW + lovasz::kThreads - 1) / lovasz::kThreads), (unsigned)B);
    const dim3 block(lovasz::kThreads);
    LOVASZ_LAUNCH(lovasz::errors_kernel, pix, block, s, probas, labels, at<uint32_t>(ws, L.keys[0]),
                  at<uint32_t>(ws, L.pays[0]), C, L.HW, L.L, ignore, ignore_none ? 1 : 0, per_image ? 1 : 0);
    lovasz::sort_scan_finalize(ws, L, B, C, per_image, sel, loss, n_kept, s);
    return launched("forward");
}

__attribute__((visibility("default"))) int ccnet_lovasz_backward_f32(const float *grad_out, float *grad_probas,
                                                                     const void *workspace, size_t workspace_bytes, int B,
                                                                     int C, int H, int W, int per_image, void *stream) {
    Layout L;
    if (!layout(B, C, H, W, per_image, L))
        return fail(-1, "backward: bad shape B=%d C=%d H=%d W=%d per_image=%d", B, C, H, W, per_image);
    if (!grad_out || !grad_probas || !workspace) return fail(-2, "backward: NULL grad_out, grad_probas or workspace");
    if (workspace_bytes < L.total)
        return fail(-3, "backward: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
    void *ws = const_cast<void *>(workspace);
    const dim3 pix((unsigned)((L.HW + lovasz::kThreads - 1) / lovasz::kThreads), (unsigned)B);
    LOVASZ_LAUNCH(lovasz::backward_kernel, pix, dim3(lovasz::kThreads), static_cast<hipStream_t>(stream), grad_out,
                  grad_probas, (const float *)at<float>(ws, L.g), (const int *)at<int>(ws, L.seg_mult),
                  (const int *)at<int>(ws, L.seg_den), B, C, L.HW, L.L, per_image ? 1 : 0);
    return launched("backward");
}

}  // extern "C"
