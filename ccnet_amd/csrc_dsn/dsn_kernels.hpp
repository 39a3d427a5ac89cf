// dsn_kernels.hpp -- the three kernels behind include/ccnet_dsn.h.
//
//   forward     one thread per full-resolution pixel, consecutive lanes along W (the int64 target, the largest input, is read
//               once and coalesced); both heads in the same launch.  Per head: the C logits interpolated from their four
//               low-resolution taps (PyTorch's align_corners=True arithmetic, fp32, its order) through an online softmax;
//               lse - z_target of valid pixels; the per-pixel log-sum-exp per head and the two-byte label go to the
//               workspace, one (sum per head, valid, out-of-range) partial per block
//   finalize    one workgroup: the block partials summed in a fixed order (double), CE_k = sum_k / valid, the weighted loss
//   backward    a gather, one thread per low-resolution gradient element (b, head, c, y, x): the thread holds the 3 x 3
//               low-resolution patch of its class around (y, x) in registers, walks the full-resolution pixels whose
//               footprint touches (y, x), recomputes their gradient g = softmax - onehot from the patch and the saved
//               log-sum-exp, and sums Wy * (sum of Wx * g) in a fixed order.  No atomics of any kind, no LDS, no barrier.
// Which full-resolution pixels touch (y, x) is decided by evaluating axis_taps -- the forward's own fp32 expressions -- over
// a conservative candidate range; no closed form decides membership.
#pragma once
#include <dsn_platform.hpp>

#include <math.h>
#include <stdint.h>

namespace dsn {

constexpr int kPixThreads = 256;       // forward / backward blocks
constexpr int kFinalThreads = 256;
constexpr int kMaxClasses = 256;       // the bound of CCNET_EVAL_MAX_CLASSES

struct Scalars {                       // device-side results of one forward, read by the backward
    int valid;
    int out_of_range;
    int pad[2];
};

struct Taps {                          // one axis of the bilinear footprint of an output index
    int i0, i1;
    float l0, l1;
};

// PyTorch's align_corners=True source index and weights, fp32 (scale = (float)(n_in - 1) / (n_out - 1), 0 when n_out == 1)
__device__ __forceinline__ Taps axis_taps(float scale, int o, int n_in) {
    Taps t;
    const float src = scale * (float)o;
    t.i0 = (int)src;
    if (t.i0 > n_in - 1) t.i0 = n_in - 1;                   // (never taken at the supported sizes: keeps every index in range)
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}

__device__ __forceinline__ float bilinear(const Taps &ty, const Taps &tx, float v00, float v01, float v10, float v11) {
    return ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
}

// the output indices o in [lo, hi] that can have i0 == i or i1 == i: real-valued o in ((i - 1) / scale, (i + 1) / scale),
// widened by one on each side (the fp32 src is within 1e-7 relative of the real one and n_out <= 2^20); axis_taps decides
__device__ __forceinline__ void candidates(int i, int n_in, int n_out, int &lo, int &hi) {
    lo = 0;
    hi = n_out - 1;
    if (n_in > 1 && n_out > 1) {
        const double inv = (double)(n_out - 1) / (double)(n_in - 1);
        const int a = (int)floor((double)(i - 1) * inv) - 1, b = (int)ceil((double)(i + 1) * inv) + 1;
        if (a > lo) lo = a;
        if (b < hi) hi = b;
    }
}

// one head of one full-resolution pixel: online softmax over the C interpolated logits; o.. are the four taps' offsets in a
// (h, w) plane, `plane` = h * w
__device__ __forceinline__ void pixel_head(const float *img, int C, int plane, int o00, int o01, int o10, int o11,
                                           const Taps &ty, const Taps &tx, int t, float &lse, float &zt) {
    float m = bilinear(ty, tx, img[o00], img[o01], img[o10], img[o11]);
    float s = 1.f;
    zt = m;
    for (int c = 1; c < C; ++c) {
        const float *pc = img + (size_t)c * plane;
        const float z = bilinear(ty, tx, pc[o00], pc[o01], pc[o10], pc[o11]);
        if (c == t) zt = z;
        if (z > m) {
            s = s * expf(m - z) + 1.f;
            m = z;
        } else {
            s += expf(z - m);
        }
    }
    lse = m + logf(s);
}

__global__ __launch_bounds__(kPixThreads) void forward_kernel(const float *logits0, const float *logits1, const int64_t *target,
                                                              float *part_sum, int *part_cnt, float *pix_lse, int16_t *pix_tgt,
                                                              int C, int h, int w, int H, int W, int N, int heads, float sh,
                                                              float sw, long long ignore) {
    __shared__ float wsum[2][kPixThreads / kWave];
    __shared__ int wcnt[2][kPixThreads / kWave];
    const int i = blockIdx.x * kPixThreads + threadIdx.x;
    float nll[2] = {0.f, 0.f};
    int valid = 0, oor = 0;
    if (i < N) {
        const int HW = H * W, b = i / HW, r = i - b * HW, oy = r / W, ox = r - oy * W;
        const long long lab = target[i];
        const bool in_range = lab >= 0 && lab < C;
        valid = lab != ignore && in_range;
        oor = lab != ignore && !in_range;
        float lse[2] = {0.f, 0.f};
        if (valid) {
            const int t = (int)lab, plane = h * w;
            const Taps ty = axis_taps(sh, oy, h), tx = axis_taps(sw, ox, w);
            const int o00 = ty.i0 * w + tx.i0, o01 = ty.i0 * w + tx.i1, o10 = ty.i1 * w + tx.i0, o11 = ty.i1 * w + tx.i1;
            float zt;
            pixel_head(logits0 + (size_t)b * C * plane, C, plane, o00, o01, o10, o11, ty, tx, t, lse[0], zt);
            nll[0] = lse[0] - zt;
            if (heads == 2) {
                pixel_head(logits1 + (size_t)b * C * plane, C, plane, o00, o01, o10, o11, ty, tx, t, lse[1], zt);
                nll[1] = lse[1] - zt;
            }
        }
        pix_lse[i] = lse[0];
        if (heads == 2) pix_lse[(size_t)N + i] = lse[1];
        pix_tgt[i] = valid ? (int16_t)lab : (int16_t)-1;
    }
    nll[0] = wave_sum(nll[0]);
    nll[1] = wave_sum(nll[1]);
    valid = wave_sum(valid);
    oor = wave_sum(oor);
    if (lane_id() == 0) {
        wsum[0][threadIdx.x / kWave] = nll[0];
        wsum[1][threadIdx.x / kWave] = nll[1];
        wcnt[0][threadIdx.x / kWave] = valid;
        wcnt[1][threadIdx.x / kWave] = oor;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a0 = 0.f, a1 = 0.f;
        int k0 = 0, k1 = 0;
        for (int v = 0; v < kPixThreads / kWave; ++v) {
            a0 += wsum[0][v];
            a1 += wsum[1][v];
            k0 += wcnt[0][v];
            k1 += wcnt[1][v];
        }
        part_sum[2 * blockIdx.x] = a0;
        part_sum[2 * blockIdx.x + 1] = a1;
        part_cnt[2 * blockIdx.x] = k0;
        part_cnt[2 * blockIdx.x + 1] = k1;
    }
}

__global__ __launch_bounds__(kFinalThreads) void finalize_kernel(const float *part_sum, const int *part_cnt, int nblk, int heads,
                                                                 float weight0, float weight1, Scalars *sc, float *loss,
                                                                 float *head_loss, int *counts) {
    __shared__ double wsum[2][kFinalThreads / kWave];
    __shared__ int wcnt[2][kFinalThreads / kWave];
    double a0 = 0.0, a1 = 0.0;
    int k0 = 0, k1 = 0;
    for (int i = threadIdx.x; i < nblk; i += kFinalThreads) {
        a0 += part_sum[2 * i];
        a1 += part_sum[2 * i + 1];
        k0 += part_cnt[2 * i];
        k1 += part_cnt[2 * i + 1];
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    k0 = wave_sum(k0);
    k1 = wave_sum(k1);
    if (lane_id() == 0) {
        wsum[0][threadIdx.x / kWave] = a0;
        wsum[1][threadIdx.x / kWave] = a1;
        wcnt[0][threadIdx.x / kWave] = k0;
        wcnt[1][threadIdx.x / kWave] = k1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s0 = 0.0, s1 = 0.0;
        int n = 0, m = 0;
        for (int v = 0; v < kFinalThreads / kWave; ++v) {
            s0 += wsum[0][v];
            s1 += wsum[1][v];
            n += wcnt[0][v];
            m += wcnt[1][v];
        }
        sc->valid = n;
        sc->out_of_range = m;
        const float ce0 = (float)(s0 / (double)n);            // 0 / 0 = NaN when no pixel is valid, as F.cross_entropy
        const float ce1 = heads == 2 ? (float)(s1 / (double)n) : 0.f;
        *loss = heads == 2 ? weight0 * ce0 + weight1 * ce1 : weight0 * ce0;
        if (head_loss) {
            head_loss[0] = ce0;
            head_loss[1] = ce1;
        }
        if (counts) {
            counts[0] = n;
            counts[1] = m;
        }
    }
}

__device__ __forceinline__ float pick3(const float (&v)[3], int i) { return i == 0 ? v[0] : (i == 1 ? v[1] : v[2]); }

// grid (ceil(h * w / kPixThreads), C, B * heads): consecutive lanes along the low-resolution row, so the store is coalesced
__global__ __launch_bounds__(kPixThreads) void backward_kernel(const float *grad_out, const float *logits0, const float *logits1,
                                                               float *grad0, float *grad1, float weight0, float weight1,
                                                               const float *pix_lse, const int16_t *pix_tgt, const Scalars *sc,
                                                               int C, int h, int w, int H, int W, int N, int heads, float sh,
                                                               float sw) {
    const int p = blockIdx.x * kPixThreads + threadIdx.x;
    if (p >= h * w) return;
    const int c = blockIdx.y, b = blockIdx.z / heads, k = blockIdx.z - b * heads;
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
    int ylo, yhi, xlo, xhi;
    candidates(y, h, H, ylo, yhi);
    candidates(x, w, W, xlo, xhi);
    float acc = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
        const Taps ty = axis_taps(sh, oy, h);
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
            const Taps tx = axis_taps(sw, ox, w);
            if (tx.i0 != x && tx.i1 != x) continue;
            const int t = tgt[oy * W + ox];
            if (t < 0) continue;
            const float wx = (tx.i0 == x ? tx.l0 : 0.f) + (tx.i1 == x ? tx.l1 : 0.f);
            const int s0 = tx.i0 - (x - 1), s1 = tx.i1 - (x - 1);
            const float z = bilinear(ty, tx, pick3(top, s0), pick3(top, s1), pick3(bot, s0), pick3(bot, s1));
            const float prob = expf(z - lse[oy * W + ox]);
            row += wx * (t == c ? prob - 1.f : prob);
        }
        acc += wy * row;
    }
    const int n = sc->valid;
    const float scale = n > 0 ? grad_out[0] * (k ? weight1 : weight0) / (float)n : 0.f;   // nothing valid: zero, not 0 * inf
    (k ? grad1 : grad0)[at + p] = acc * scale;
}

}  // namespace dsn
