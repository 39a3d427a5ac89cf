// lovasz_api.hip -- the C ABI of include/ccnet_lovasz.h (libccnet_lovasz.so): argument checks, workspace layout, launches.
// Every launch goes on the caller's stream and nothing waits for the device.
#include "ccnet_lovasz.h"

#include "lovasz_kernels.hpp"

#define CCNET_ERROR_PREFIX "ccnet_lovasz: "
#include "../csrc_common/ccnet_host.hpp"

namespace {

struct Layout {
    int HW, L, S, nt;
    size_t E;                                                  // sort elements: segments x segment length
    size_t keys[2], pays[2], g, counts, blk_fg, blk_valid, blk_loss, seg_gts, seg_nvalid, seg_loss, seg_mult, seg_den,
        total;
};

bool layout(int B, int C, int H, int W, int per_image, Layout &L) {
    if (B < 1 || C < 2 || C > lovasz::kMaxClasses || H < 1 || W < 1) return false;
    const long long hw = (long long)H * W, len = per_image ? hw : hw * B, segs = per_image ? (long long)B * C : C;
    if (len > lovasz::kMaxSegment || B > 65535 || segs > 65535) return false;
    L.HW = (int)hw;
    L.L = (int)len;
    L.S = (int)segs;
    L.nt = (L.L + lovasz::kTile - 1) / lovasz::kTile;
    L.E = (size_t)L.S * L.L;
    const size_t tiles = (size_t)L.S * L.nt;
    size_t o = 0;
    for (int i = 0; i < 2; ++i) {
        L.keys[i] = o; o += align256(4 * L.E);
        L.pays[i] = o; o += align256(4 * L.E);
    }
    L.g = o;          o += align256(4 * L.E);
    L.counts = o;     o += align256(4 * tiles * lovasz::kRadix);
    L.blk_fg = o;     o += align256(4 * tiles);
    L.blk_valid = o;  o += align256(4 * tiles);
    L.blk_loss = o;   o += align256(8 * tiles);
    L.seg_gts = o;    o += align256(4 * (size_t)L.S);
    L.seg_nvalid = o; o += align256(4 * (size_t)L.S);
    L.seg_loss = o;   o += align256(8 * (size_t)L.S);
    L.seg_mult = o;   o += align256(4 * (size_t)L.S);
    L.seg_den = o;    o += align256(4 * (size_t)L.S);
    L.total = o;
    return true;
}

}  // namespace

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
    lovasz::ClassSel sel = {};
    for (int c = 0; c < C; ++c) sel.weight[c] = class_weights ? class_weights[c] : 1;
    sel.present_only = present_only ? 1 : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    void *ws = workspace;
    const dim3 pix((unsigned)((L.HW + lovasz::kThreads - 1) / lovasz::kThreads), (unsigned)B);
    const dim3 tiles((unsigned)L.nt, (unsigned)L.S), block(lovasz::kThreads);
    unsigned *counts = at<unsigned>(ws, L.counts);
    LOVASZ_LAUNCH(lovasz::errors_kernel, pix, block, s, probas, labels, at<uint32_t>(ws, L.keys[0]),
                  at<uint32_t>(ws, L.pays[0]), C, L.HW, L.L, ignore, ignore_none ? 1 : 0, per_image ? 1 : 0);
    for (int pass = 0; pass < 4; ++pass) {
        const int src = pass & 1, dst = src ^ 1, shift = 8 * pass;
        LOVASZ_LAUNCH(lovasz::radix_hist_kernel, tiles, block, s, (const uint32_t *)at<uint32_t>(ws, L.keys[src]), counts,
                      L.L, L.nt, shift);
        LOVASZ_LAUNCH(lovasz::radix_offsets_kernel, dim3((unsigned)L.S), block, s, counts, L.nt);
        LOVASZ_LAUNCH(lovasz::radix_scatter_kernel, tiles, block, s, (const uint32_t *)at<uint32_t>(ws, L.keys[src]),
                      (const uint32_t *)at<uint32_t>(ws, L.pays[src]), at<uint32_t>(ws, L.keys[dst]),
                      at<uint32_t>(ws, L.pays[dst]), (const unsigned *)counts, L.L, L.nt, shift);
    }
    // four passes: the sorted keys and payloads are back in buffer 0
    const uint32_t *keys = at<uint32_t>(ws, L.keys[0]), *pays = at<uint32_t>(ws, L.pays[0]);
    LOVASZ_LAUNCH(lovasz::scan_count_kernel, tiles, block, s, keys, pays, at<unsigned>(ws, L.blk_fg),
                  at<unsigned>(ws, L.blk_valid), L.L, L.nt);
    LOVASZ_LAUNCH(lovasz::scan_offsets_kernel, dim3((unsigned)L.S), block, s, at<unsigned>(ws, L.blk_fg),
                  (const unsigned *)at<unsigned>(ws, L.blk_valid), at<unsigned>(ws, L.seg_gts),
                  at<unsigned>(ws, L.seg_nvalid), L.nt);
    LOVASZ_LAUNCH(lovasz::scan_grad_kernel, tiles, block, s, keys, pays, (const unsigned *)at<unsigned>(ws, L.blk_fg),
                  (const unsigned *)at<unsigned>(ws, L.seg_gts), (const unsigned *)at<unsigned>(ws, L.seg_nvalid),
                  at<float>(ws, L.g), at<double>(ws, L.blk_loss), L.L, L.nt);
    LOVASZ_LAUNCH(lovasz::finalize_kernel, dim3(1), block, s, (const double *)at<double>(ws, L.blk_loss),
                  (const unsigned *)at<unsigned>(ws, L.seg_gts), (const unsigned *)at<unsigned>(ws, L.seg_nvalid),
                  at<double>(ws, L.seg_loss), at<int>(ws, L.seg_mult), at<int>(ws, L.seg_den), L.nt, B, C,
                  per_image ? 1 : 0, sel, loss, n_kept);
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
