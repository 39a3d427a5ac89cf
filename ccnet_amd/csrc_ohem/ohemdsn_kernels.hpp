// ohemdsn_kernels.hpp -- the kernels behind include/ccnet_ohemdsn.h: OHEM cross-entropy on the main head + 0.4 x cross-entropy
// on the DSN head, both on low-resolution logits that are up-sampled as they are read.
//
//   zoom_keys   one thread per zoomed pixel: ohem::zoom_key (label pick, taps, double weights, key) with the probability of a
//               full-resolution tap computed on the spot: target_prob below, over the C logits interpolated at that pixel
//   select      ohem::select_kernel, unchanged: the k-th smallest key and the threshold
//   forward     one thread per full-resolution pixel, consecutive lanes along W, the target read once for both heads.  Head 0:
//               target_prob again -- the function the keys were made of, so a pixel and a key made of its value compare
//               bit-equal -- and keep = valid && p <= threshold.  Head 1: dsn::pixel_head.  A log-sum-exp per head and the
//               two-byte label with the kept flag go to the workspace, one partial per block
//   finalize    one workgroup: the partials summed in a fixed order (double), CE0 = sum0 / kept, CE1 = sum1 / valid
//   backward    the gather of dsn::backward_kernel (same grid, 3 x 3 register patch, membership by dsn::axis_taps, fixed
//               order; the threads numbered class-fastest, see there): head 0 skips pixels that were not kept and scales by
//               grad_out / kept, head 1 by 0.4 * grad_out / valid
// The up-sample arithmetic (axis_taps, bilinear, candidates, pick3) is dsn::'s and the zoom's is ohem::'s; neither is restated.
#pragma once
#include "ohem_kernels.hpp"

#include <dsn_kernels.hpp>

namespace ohemdsn {

using dsn::kWave;
using dsn::lane_id;
using dsn::wave_sum;

constexpr int kPixThreads = 256;       // zoom / forward / backward blocks
constexpr int kFinalThreads = 256;
constexpr int kKeptBit = 0x100;        // labels are below 256 (dsn::kMaxClasses): bit 8 of the saved label says "kept by head 0"
constexpr float kAuxWeight = 0.4f;     // loss/criterion.py:56

struct Scalars {                       // device-side results of one forward, read by the backward
    int kept;
    int valid;
    int out_of_range;
    int pad;
};

struct Foot {                          // the bilinear footprint of one full-resolution pixel in a (h, w) plane
    dsn::Taps ty, tx;
    int o00, o01, o10, o11;
};

__device__ __forceinline__ Foot footprint(float sh, float sw, int oy, int ox, int h, int w) {
    Foot f;
    f.ty = dsn::axis_taps(sh, oy, h);
    f.tx = dsn::axis_taps(sw, ox, w);
    f.o00 = f.ty.i0 * w + f.tx.i0;
    f.o01 = f.ty.i0 * w + f.tx.i1;
    f.o10 = f.ty.i1 * w + f.tx.i0;
    f.o11 = f.ty.i1 * w + f.tx.i1;
    return f;
}

__device__ __forceinline__ float logit_at(const float *pc, const Foot &f) {
    return dsn::bilinear(f.ty, f.tx, pc[f.o00], pc[f.o01], pc[f.o10], pc[f.o11]);
}

// the softmax probability of class t at one full-resolution pixel of one image (`img`: its (C, h, w) logits), two passes like
// ohem::target_prob (max, then the sum of exp(z - max) in class order) over the interpolated logits; also the pixel's
// log-sum-exp and its target logit.  The one definition of p_target: the keys and the keep decision both call it.
__device__ __forceinline__ float target_prob(const float *img, int C, int plane, const Foot &f, int t, float &lse, float &zt) {
    float m = logit_at(img, f);
    for (int c = 1; c < C; ++c) m = fmaxf(m, logit_at(img + (size_t)c * plane, f));
    float s = 0.f;
    zt = 0.f;
    for (int c = 0; c < C; ++c) {
        const float z = logit_at(img + (size_t)c * plane, f);
        if (c == t) zt = z;
        s += expf(z - m);
    }
    lse = m + logf(s);
    return expf(zt - m) / s;
}

__global__ __launch_bounds__(kPixThreads) void zoom_keys_kernel(const float *logits0, const int64_t *target, uint32_t *keys,
                                                                int B, int C, int h, int w, int H, int W, int ho, int wo,
                                                                double zy, double zx, float sh, float sw, long long ignore) {
    const int i = blockIdx.x * kPixThreads + threadIdx.x;
    if (i >= B * ho * wo) return;
    const int b = i / (ho * wo), r = i - b * (ho * wo), oy = r / wo, ox = r - oy * wo;
    const int plane = h * w;
    const float *img = logits0 + (size_t)b * C * plane;
    keys[i] = ohem::zoom_key(target, b, C, H, W, oy, ox, zy, zx, ignore, [&](int t, int y, int x) {
        float lse, zt;
        return target_prob(img, C, plane, footprint(sh, sw, y, x, h, w), t, lse, zt);
    });
}

__global__ __launch_bounds__(kPixThreads) void forward_kernel(const float *logits0, const float *logits1, const int64_t *target,
                                                              const ohem::Scalars *sel, float *part_sum, int *part_cnt,
                                                              float *pix_lse, int16_t *pix_tgt, int C, int h, int w, int H,
                                                              int W, int N, int heads, float sh, float sw, long long ignore) {
    __shared__ float wsum[2][kPixThreads / kWave];
    __shared__ int wcnt[3][kPixThreads / kWave];
    const int i = blockIdx.x * kPixThreads + threadIdx.x;
    float nll[2] = {0.f, 0.f};
    int keep = 0, valid = 0, oor = 0;
    if (i < N) {
        const int HW = H * W, b = i / HW, r = i - b * HW, oy = r / W, ox = r - oy * W;
        const long long lab = target[i];
        const bool in_range = lab >= 0 && lab < C;
        valid = lab != ignore && in_range;
        oor = lab != ignore && !in_range;
        float lse[2] = {0.f, 0.f};
        if (valid) {
            const int t = (int)lab, plane = h * w;
            const Foot f = footprint(sh, sw, oy, ox, h, w);
            float zt;
            const float p = target_prob(logits0 + (size_t)b * C * plane, C, plane, f, t, lse[0], zt);
            keep = p <= sel->threshold;
            if (keep) nll[0] = lse[0] - zt;
            if (heads == 2) {
                dsn::pixel_head(logits1 + (size_t)b * C * plane, C, plane, f.o00, f.o01, f.o10, f.o11, f.ty, f.tx, t, lse[1], zt);
                nll[1] = lse[1] - zt;
            }
        }
        pix_lse[i] = lse[0];
        if (heads == 2) pix_lse[(size_t)N + i] = lse[1];
        pix_tgt[i] = valid ? (int16_t)((int)lab | (keep ? kKeptBit : 0)) : (int16_t)-1;
    }
    nll[0] = wave_sum(nll[0]);
    nll[1] = wave_sum(nll[1]);
    keep = wave_sum(keep);
    valid = wave_sum(valid);
    oor = wave_sum(oor);
    if (lane_id() == 0) {
        const int v = threadIdx.x / kWave;
        wsum[0][v] = nll[0];
        wsum[1][v] = nll[1];
        wcnt[0][v] = keep;
        wcnt[1][v] = valid;
        wcnt[2][v] = oor;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a0 = 0.f, a1 = 0.f;
        int k0 = 0, k1 = 0, k2 = 0;
        for (int v = 0; v < kPixThreads / kWave; ++v) {
            a0 += wsum[0][v];
            a1 += wsum[1][v];
            k0 += wcnt[0][v];
            k1 += wcnt[1][v];
            k2 += wcnt[2][v];
        }
        part_sum[2 * blockIdx.x] = a0;
        part_sum[2 * blockIdx.x + 1] = a1;
        part_cnt[3 * blockIdx.x] = k0;
        part_cnt[3 * blockIdx.x + 1] = k1;
        part_cnt[3 * blockIdx.x + 2] = k2;
    }
}

__global__ __launch_bounds__(kFinalThreads) void finalize_kernel(const float *part_sum, const int *part_cnt, int nblk, int heads,
                                                                 const ohem::Scalars *sel, Scalars *sc, float *loss,
                                                                 float *head_loss, int *counts) {
    __shared__ double wsum[2][kFinalThreads / kWave];
    __shared__ int wcnt[3][kFinalThreads / kWave];
    double a0 = 0.0, a1 = 0.0;
    int k0 = 0, k1 = 0, k2 = 0;
    for (int i = threadIdx.x; i < nblk; i += kFinalThreads) {
        a0 += part_sum[2 * i];
        a1 += part_sum[2 * i + 1];
        k0 += part_cnt[3 * i];
        k1 += part_cnt[3 * i + 1];
        k2 += part_cnt[3 * i + 2];
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    k0 = wave_sum(k0);
    k1 = wave_sum(k1);
    k2 = wave_sum(k2);
    if (lane_id() == 0) {
        const int v = threadIdx.x / kWave;
        wsum[0][v] = a0;
        wsum[1][v] = a1;
        wcnt[0][v] = k0;
        wcnt[1][v] = k1;
        wcnt[2][v] = k2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s0 = 0.0, s1 = 0.0;
        int kept = 0, valid = 0, oor = 0;
        for (int v = 0; v < kFinalThreads / kWave; ++v) {
            s0 += wsum[0][v];
            s1 += wsum[1][v];
            kept += wcnt[0][v];
            valid += wcnt[1][v];
            oor += wcnt[2][v];
        }
        sc->kept = kept;
        sc->valid = valid;
        sc->out_of_range = oor;
        const float ce0 = (float)(s0 / (double)kept);         // 0 / 0 = NaN when nothing is kept, as F.cross_entropy
        const float ce1 = heads == 2 ? (float)(s1 / (double)valid) : 0.f;
        *loss = heads == 2 ? ce0 + ce1 * kAuxWeight : ce0;
        if (head_loss) {
            head_loss[0] = ce0;
            head_loss[1] = ce1;
        }
        if (counts) {
            counts[0] = kept;
            counts[1] = valid;
            counts[2] = sel->num_valid;
            counts[3] = oor;
        }
    }
}

// grid (ceil(h * w / kPixThreads), C, B * heads), dsn::backward_kernel's; the threads of one (image, head) slice of it are
// numbered with the class fastest: the lanes of a wave then hold the 19 classes of three or four neighbouring low-resolution
// pixels and walk the same full-resolution pixels together, so the label and the log-sum-exp -- two loads per step of the
// walk -- come from one or two cache lines a wave where a wave of 64 neighbouring pixels touches sixteen and more.  The
// nine patch loads and the one store of a thread are strided by a plane instead; they are outside the walk.
__global__ __launch_bounds__(kPixThreads) void backward_kernel(const float *grad_out, const float *logits0, const float *logits1,
                                                               float *grad0, float *grad1, const float *pix_lse,
                                                               const int16_t *pix_tgt, const Scalars *sc, int C, int h, int w,
                                                               int H, int W, int N, int heads, float sh, float sw) {
    const unsigned lin = (blockIdx.y * gridDim.x + blockIdx.x) * kPixThreads + threadIdx.x;   // below C * (h * w + 255) < 2^32
    const int p = (int)(lin / (unsigned)C), c = (int)(lin - (unsigned)p * (unsigned)C);
    if (p >= h * w) return;
    const int b = blockIdx.z / heads, k = blockIdx.z - b * heads;
    const int y = p / w, x = p - y * w;
    const size_t at = ((size_t)b * C + c) * (size_t)(h * w);
    const float *img = (k ? logits1 : logits0) + at;
    float patch[3][3];                                       // rows y-1 .. y+1, columns x-1 .. x+1 (clamped ones are never picked)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int yy = y - 1 + r < 0 ? 0 : (y - 1 + r > h - 1 ? h - 1 : y - 1 + r);
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int xx = x - 1 + s < 0 ? 0 : (x - 1 + s > w - 1 ? w - 1 : x - 1 + s);
            patch[r][s] = img[yy * w + xx];
        }
    }
    const float *lse = pix_lse + (size_t)k * N + (size_t)b * H * W;
    const int16_t *tgt = pix_tgt + (size_t)b * H * W;
    const int need = k ? 0 : kKeptBit;                       // head 0 takes kept pixels only, head 1 every valid one
    int ylo, yhi, xlo, xhi;
    dsn::candidates(y, h, H, ylo, yhi);
    dsn::candidates(x, w, W, xlo, xhi);
    float acc = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
        const dsn::Taps ty = dsn::axis_taps(sh, oy, h);
        if (ty.i0 != y && ty.i1 != y) continue;
        const float wy = (ty.i0 == y ? ty.l0 : 0.f) + (ty.i1 == y ? ty.l1 : 0.f);   // i0 == i1 == h-1: both weights land here
        const int r0 = ty.i0 - (y - 1), r1 = ty.i1 - (y - 1);
        float top[3], bot[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            top[s] = r0 == 0 ? patch[0][s] : (r0 == 1 ? patch[1][s] : patch[2][s]);
            bot[s] = r1 == 0 ? patch[0][s] : (r1 == 1 ? patch[1][s] : patch[2][s]);
        }
        float row = 0.f;
        for (int ox = xlo; ox <= xhi; ++ox) {
            const dsn::Taps tx = dsn::axis_taps(sw, ox, w);
            if (tx.i0 != x && tx.i1 != x) continue;
            const int t = tgt[oy * W + ox];
            if (t < 0 || (t & need) != need) continue;
            const float wx = (tx.i0 == x ? tx.l0 : 0.f) + (tx.i1 == x ? tx.l1 : 0.f);
            const int s0 = tx.i0 - (x - 1), s1 = tx.i1 - (x - 1);
            const float z = dsn::bilinear(ty, tx, dsn::pick3(top, s0), dsn::pick3(top, s1), dsn::pick3(bot, s0), dsn::pick3(bot, s1));
            const float prob = expf(z - lse[oy * W + ox]);
            row += wx * ((t & (kKeptBit - 1)) == c ? prob - 1.f : prob);
        }
        acc += wy * row;
    }
    const int n = k ? sc->valid : sc->kept;
    const float scale = n > 0 ? grad_out[0] * (k ? kAuxWeight : 1.f) / (float)n : 0.f;   // a zero count: zero, not 0 * inf
    (k ? grad1 : grad0)[at + p] = acc * scale;
}

}  // namespace ohemdsn
