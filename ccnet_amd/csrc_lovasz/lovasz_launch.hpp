// lovasz_launch.hpp -- the host side that the two translation units of this directory share (lovasz_api.hip and
// celovasz_api.hip): the layout of the Lovász workspace and the launch sequence from sort keys to the loss.  A unit includes
// it after lovasz_kernels.hpp and ../csrc_common/ccnet_host.hpp (align256, at); what produces the keys and payloads
// (lovasz::errors_kernel there, celovasz::pixel_errors_kernel here) and what consumes g is the unit's own.
#pragma once

namespace lovasz {

struct Layout {
    int HW, L, S, nt;
    size_t E;                                                  // sort elements: segments x segment length
    size_t keys[2], pays[2], g, counts, blk_fg, blk_valid, blk_loss, seg_gts, seg_nvalid, seg_loss, seg_mult, seg_den,
        total;
};

inline bool layout(int B, int C, int H, int W, int per_image, Layout &L) {
    if (B < 1 || C < 2 || C > kMaxClasses || H < 1 || W < 1) return false;
    const long long hw = (long long)H * W, len = per_image ? hw : hw * B, segs = per_image ? (long long)B * C : C;
    if (len > kMaxSegment || B > 65535 || segs > 65535) return false;
    L.HW = (int)hw;
    L.L = (int)len;
    L.S = (int)segs;
    L.nt = (L.L + kTile - 1) / kTile;
    L.E = (size_t)L.S * L.L;
    const size_t tiles = (size_t)L.S * L.nt;
    size_t o = 0;
    for (int i = 0; i < 2; ++i) {
        L.keys[i] = o; o += align256(4 * L.E);
        L.pays[i] = o; o += align256(4 * L.E);
    }
    L.g = o;          o += align256(4 * L.E);
    L.counts = o;     o += align256(4 * tiles * kRadix);
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

inline ClassSel class_sel(const unsigned char *class_weights, int C, int present_only) {
    ClassSel sel = {};
    for (int c = 0; c < C; ++c) sel.weight[c] = class_weights ? class_weights[c] : 1;
    sel.present_only = present_only ? 1 : 0;
    return sel;
}

// keys and payloads in buffer 0 of `ws` -> sorted (four radix passes), scanned (g at every pixel's slot, the per-tile loss
// partials), finalized (seg_mult, seg_den, the loss and the kept class count)
inline void sort_scan_finalize(void *ws, const Layout &L, int B, int C, int per_image, const ClassSel &sel, float *loss,
                               int *n_kept, hipStream_t s) {
    const dim3 tiles((unsigned)L.nt, (unsigned)L.S), block(kThreads);
    unsigned *counts = at<unsigned>(ws, L.counts);
    for (int pass = 0; pass < 4; ++pass) {
        const int src = pass & 1, dst = src ^ 1, shift = 8 * pass;
        LOVASZ_LAUNCH(radix_hist_kernel, tiles, block, s, (const uint32_t *)at<uint32_t>(ws, L.keys[src]), counts, L.L, L.nt,
                      shift);
        LOVASZ_LAUNCH(radix_offsets_kernel, dim3((unsigned)L.S), block, s, counts, L.nt);
        LOVASZ_LAUNCH(radix_scatter_kernel, tiles, block, s, (const uint32_t *)at<uint32_t>(ws, L.keys[src]),
                      (const uint32_t *)at<uint32_t>(ws, L.pays[src]), at<uint32_t>(ws, L.keys[dst]),
                      at<uint32_t>(ws, L.pays[dst]), (const unsigned *)counts, L.L, L.nt, shift);
    }
    // four passes: the sorted keys and payloads are back in buffer 0
    const uint32_t *keys = at<uint32_t>(ws, L.keys[0]), *pays = at<uint32_t>(ws, L.pays[0]);
    LOVASZ_LAUNCH(scan_count_kernel, tiles, block, s, keys, pays, at<unsigned>(ws, L.blk_fg), at<unsigned>(ws, L.blk_valid),
                  L.L, L.nt);
    LOVASZ_LAUNCH(scan_offsets_kernel, dim3((unsigned)L.S), block, s, at<unsigned>(ws, L.blk_fg),
                  (const unsigned *)at<unsigned>(ws, L.blk_valid), at<unsigned>(ws, L.seg_gts),
                  at<unsigned>(ws, L.seg_nvalid), L.nt);
    LOVASZ_LAUNCH(scan_grad_kernel, tiles, block, s, keys, pays, (const unsigned *)at<unsigned>(ws, L.blk_fg),
                  (const unsigned *)at<unsigned>(ws, L.seg_gts), (const unsigned *)at<unsigned>(ws, L.seg_nvalid),
                  at<float>(ws, L.g), at<double>(ws, L.blk_loss), L.L, L.nt);
    LOVASZ_LAUNCH(finalize_kernel, dim3(1), block, s, (const double *)at<double>(ws, L.blk_loss),
                  (const unsigned *)at<unsigned>(ws, L.seg_gts), (const unsigned *)at<unsigned>(ws, L.seg_nvalid),
                  at<double>(ws, L.seg_loss), at<int>(ws, L.seg_mult), at<int>(ws, L.seg_den), L.nt, B, C,
                  per_image ? 1 : 0, sel, loss, n_kept);
}

}  // namespace lovasz
