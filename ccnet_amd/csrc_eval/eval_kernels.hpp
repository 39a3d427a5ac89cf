// eval_kernels.hpp -- the one kernel behind include/ccnet_eval.h.
//
//   sliding   grid (pixel blocks, N), 256 threads, 4096 pixels a workgroup (16 a thread, consecutive threads on consecutive
//             pixels of a row: every load of labels and every store of pred / probs is coalesced along W).  Per pixel and
//             class it samples the covering tiles' 1/8-resolution logits bilinearly (PyTorch's align_corners=True
//             arithmetic), averages them per pass, averages the passes, writes the optional score and keeps the first
//             maximum; then it counts (label, pred) in a workgroup-private LDS histogram.  The 8x up-sampled tiles and the
//             full-resolution score map are never materialised unless probs is asked for: the 64 output pixels that share
//             one 2 x 2 footprint read it from L1 / L2.
//
// The histogram holds the whole C x C matrix as 16-bit counters, two to an LDS word (a workgroup counts at most 4096 pixels,
// so a counter never carries into its neighbour): C * C * 2 bytes of dynamic LDS, 724 B at C = 19, 45 000 B at C = 150,
// 128 KiB at C = 256.  Only workgroups that count allocate it.  After the pixels, each nonzero counter is added to the int64
// confusion matrix with one integer atomic: the counts are exact and independent of the order of arrival.
#pragma once
#include "eval_sample.hpp"     // TileGrid, Geometry, covers, sample, pass_mean: shared with mseval_kernels.hpp

namespace segeval {

__global__ __launch_bounds__(kThreads) void sliding_kernel(const float *tiles, TileGrid g, Geometry G, const int64_t *labels,
                                                           long long ignore, float *probs, uint8_t *pred, int64_t *conf) {
    EVAL_DYNAMIC_LDS(hist);
    const int C = G.C, HW = G.H * G.W, n = blockIdx.y;
    const int words = (C * C + 1) >> 1;
    if (conf) {
        for (int i = threadIdx.x; i < words; i += kThreads) hist[i] = 0u;
        __syncthreads();
    }
    const float *img = tiles + (size_t)n * (G.T + G.T_flip) * C * G.h * G.w;
    const int base = blockIdx.x * kPixPerBlock + threadIdx.x;
    for (int k = 0; k < kPixPerThread; ++k) {
        const int i = base + k * kThreads;
        if (i >= HW) break;
        const int y = i / G.W, x = i - y * G.W, xf = G.W - 1 - x;
        int cnt = 0, cntf = 0;
        for (int t = 0; t < G.T; ++t) {
            cnt += covers(g, G, t, y, x);
            cntf += covers(g, G, t, y, xf);
        }
        float best = 0.f;
        int arg = 0;
        for (int c = 0; c < C; ++c) {
            float s = pass_mean(img, g, G, 0, c, y, x, cnt);
            if (G.T_flip) s = 0.5f * (s + pass_mean(img, g, G, G.T, c, y, xf, cntf));
            if (probs) probs[((size_t)n * C + c) * HW + i] = s;
            if (first_maximum(c, s, best)) {          // as np.argmax: a NaN is one
                best = s;
                arg = c;
            }
        }
        if (pred) pred[(size_t)n * HW + i] = (uint8_t)arg;
        if (conf) {
            const long long lab = labels[(size_t)n * HW + i];
            if (lab != ignore && lab >= 0 && lab < C) {
                const int b = (int)lab * C + arg;
                lds_add(&hist[b >> 1], (b & 1) ? 0x10000u : 1u);
            }
        }
    }
    if (conf) {
        __syncthreads();
        for (int i = threadIdx.x; i < words; i += kThreads) {
            const unsigned v = hist[i];
            if (v & 0xffffu) global_add(conf + 2 * i, v & 0xffffu);
            if (v >> 16) global_add(conf + 2 * i + 1, v >> 16);
        }
    }
}

}  // namespace segeval
