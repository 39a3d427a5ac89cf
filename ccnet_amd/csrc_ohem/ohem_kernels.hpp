// ohem_kernels.hpp -- the five kernels behind include/ccnet_ohem.h.
//
//   zoom_keys   one thread per zoomed pixel: order-0 label pick, order-1 zoom of the label's own softmax probability
//               (double weights, scipy's tap order), written as an fp32 bit pattern; invalid labels get kInvalidKey
//   select      ONE workgroup over every key of the batch: num_valid, then a 4 x 8-bit radix select of the k-th smallest
//               key (LDS histogram, integer increments), then the threshold
//   forward     one thread per full-resolution pixel, the C logits read once (online softmax, coalesced along W): kept flag,
//               -log p_target of kept pixels, per-pixel log-sum-exp and target class for the backward, one partial
//               (sum, count) per block
//   finalize    one workgroup: the block partials summed in a fixed order (double), loss = sum / count
//   backward    one thread per pixel: grad = grad_out * (softmax - onehot) / count, the logits read once, the gradient
//               written once
// Nonnegative fp32 values order like their bit patterns, so the select works on uint32 keys.
#pragma once
#include <ohem_platform.hpp>

#include <math.h>
#include <stdint.h>
#include <string.h>

namespace ohem {

constexpr uint32_t kInvalidKey = 0xffffffffu;
constexpr int kPixThreads = 256;       // forward / backward / zoom blocks
constexpr int kSelectThreads = 1024;   // the single select workgroup
constexpr int kFinalThreads = 256;

struct Scalars {                       // device-side results of one forward, read by the backward
    float threshold;
    int kept;
    int num_valid;
    int pad;
};

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ float bits_to_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
__device__ __forceinline__ uint32_t float_to_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// one pass over the C logits of a pixel (stride `plane` floats): running max m, sum s of exp(x - m), and logit t
__device__ __forceinline__ void pixel_softmax(const float *px, int C, size_t plane, int t, float &m, float &s, float &xt) {
    m = px[0];
    s = 1.f;
    xt = m;
    for (int c = 1; c < C; ++c) {
        const float x = px[(size_t)c * plane];
        if (c == t) xt = x;
        if (x > m) {
            s = s * expf(m - x) + 1.f;
            m = x;
        } else {
            s += expf(x - m);
        }
    }
}

// the zoom's probabilities: two passes (max, then the sum of exp(x - max) in class order) like the reference's softmax, so
// the k-th value -- the threshold itself -- carries no rescaling error of the online form; these pixels are few and cached
__device__ __forceinline__ float target_prob(const float *logits, int C, int H, int W, int b, int t, int y, int x) {
    const size_t plane = (size_t)H * W;
    const float *px = logits + (size_t)b * C * plane + (size_t)y * W + x;
    float m = px[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, px[(size_t)c * plane]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(px[(size_t)c * plane] - m);
    return expf(px[(size_t)t * plane] - m) / s;
}

// scipy.ndimage.zoom's output length round(n * (1 / factor)) (ties to even) and its grid_mode=False source step (host side)
inline int zoom_len(int n, int factor) { return (int)nearbyint(n * (1.0 / factor)); }
inline double zoom_step(int n, int n_out) { return n_out > 1 ? (double)(n - 1) / (double)(n_out - 1) : 1.0; }

// the key of zoomed pixel (oy, ox) of image b: scipy's order-0 pick of the label, the four taps of its order-1 zoom, double
// weights in scipy's tap order.  `prob(t, y, x)` is the fp32 probability of class t at full-resolution pixel (y, x) of that
// image; where that comes from is the caller's (a softmax of stored logits here, of interpolated ones in ohemdsn_kernels.hpp).
template <class Prob>
__device__ __forceinline__ uint32_t zoom_key(const int64_t *labels, int b, int C, int H, int W, int oy, int ox, double zy,
                                             double zx, long long ignore, Prob prob) {
    const double cy = oy * zy, cx = ox * zx;
    const int ly = imin((int)floor(cy + 0.5), H - 1), lx = imin((int)floor(cx + 0.5), W - 1);
    const long long lab = labels[(size_t)b * H * W + (size_t)ly * W + lx];
    if (lab == ignore || lab < 0 || lab >= C) return kInvalidKey;
    const int t = (int)lab;
    const int y0 = (int)floor(cy), x0 = (int)floor(cx);
    const int y1 = imin(y0 + 1, H - 1), x1 = imin(x0 + 1, W - 1);
    const double ty = cy - y0, tx = cx - x0;
    const double wy[2] = {1.0 - ty, ty}, wx[2] = {1.0 - tx, tx};
    const int ys[2] = {y0, y1}, xs[2] = {x0, x1};
    double acc = 0.0;
    for (int a = 0; a < 2; ++a)
        for (int e = 0; e < 2; ++e) acc += (double)prob(t, ys[a], xs[e]) * wy[a] * wx[e];
    return float_to_bits((float)acc);
}

__global__ __launch_bounds__(kPixThreads) void zoom_keys_kernel(const float *logits, const int64_t *labels, uint32_t *keys,
                                                                int B, int C, int H, int W, int ho, int wo, double zy,
                                                                double zx, long long ignore) {
    const int i = blockIdx.x * kPixThreads + threadIdx.x;
    if (i >= B * ho * wo) return;
    const int b = i / (ho * wo), r = i - b * (ho * wo), oy = r / wo, ox = r - oy * wo;
    keys[i] = zoom_key(labels, b, C, H, W, oy, ox, zy, zx, ignore,
                       [&](int t, int y, int x) { return target_prob(logits, C, H, W, b, t, y, x); });
}

__global__ __launch_bounds__(kSelectThreads) void select_kernel(const uint32_t *keys, int M, int min_kept_zoomed, float thresh,
                                                                Scalars *sc, float *threshold_out, int *num_valid_out) {
    __shared__ unsigned hist[256];
    __shared__ int wave_part[kSelectThreads / kWave];
    __shared__ unsigned state[2];                     // key prefix found so far, rank left within it
    const int tid = threadIdx.x;
    int n = 0;
    for (int i = tid; i < M; i += kSelectThreads) n += keys[i] != kInvalidKey;
    n = wave_sum(n);
    if (lane_id() == 0) wave_part[tid / kWave] = n;
    __syncthreads();
    int num_valid = 0;
    for (int w = 0; w < kSelectThreads / kWave; ++w) num_valid += wave_part[w];
    float thr;
    if (min_kept_zoomed >= num_valid) {
        thr = 1.f;
    } else if (min_kept_zoomed == 0) {
        thr = thresh;
    } else {
        uint32_t prefix = 0, mask = 0, rank = (uint32_t)(min_kept_zoomed - 1);
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < M; i += kSelectThreads) {
                const uint32_t k = keys[i];
                if ((k & mask) == prefix) lds_inc(&hist[(k >> shift) & 255u]);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t below = 0, bin = 0;
                for (; bin < 255; ++bin) {
                    if (below + hist[bin] > rank) break;
                    below += hist[bin];
                }
                state[0] = prefix | (bin << shift);
                state[1] = rank - below;
            }
            __syncthreads();
            prefix = state[0];
            rank = state[1];
            mask |= 255u << shift;
            __syncthreads();
        }
        thr = fmaxf(thresh, bits_to_float(prefix));
    }
    if (tid == 0) {
        sc->threshold = thr;
        sc->num_valid = num_valid;
        if (threshold_out) *threshold_out = thr;
        if (num_valid_out) *num_valid_out = num_valid;
    }
}

__global__ __launch_bounds__(kPixThreads) void forward_kernel(const float *logits, const int64_t *labels, const Scalars *sc,
                                                              float *part_sum, int *part_cnt, float *pix_lse, int *pix_tgt,
                                                              int C, int HW, int N, long long ignore) {
    __shared__ float wsum[kPixThreads / kWave];
    __shared__ int wcnt[kPixThreads / kWave];
    const int i = blockIdx.x * kPixThreads + threadIdx.x;
    float nll = 0.f;
    int keep = 0;
    if (i < N) {
        const int b = i / HW, r = i - b * HW;
        const long long lab = labels[i];
        const bool valid = lab != ignore && lab >= 0 && lab < C;
        const int t = valid ? (int)lab : 0;
        float m, s, xt;
        pixel_softmax(logits + (size_t)b * C * HW + r, C, (size_t)HW, t, m, s, xt);
        const float lse = m + logf(s);
        // the online sum rescales, so its probability can sit a few ulp off the two-pass value the zoom ranked; near the
        // threshold the decision takes the two-pass value, so pixels whose key is the k-th (or ties it) are always kept
        const float thr = sc->threshold;
        float p = expf(xt - m) / s;
        if (valid && fabsf(p - thr) <= 1e-4f * thr) p = target_prob(logits, C, 1, HW, b, t, 0, r);
        keep = valid && p <= thr;
        if (keep) nll = lse - xt;
        pix_lse[i] = lse;
        pix_tgt[i] = keep ? t : -1;
    }
    nll = wave_sum(nll);
    keep = wave_sum(keep);
    if (lane_id() == 0) {
        wsum[threadIdx.x / kWave] = nll;
        wcnt[threadIdx.x / kWave] = keep;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f;
        int k = 0;
        for (int w = 0; w < kPixThreads / kWave; ++w) {
            a += wsum[w];
            k += wcnt[w];
        }
        part_sum[blockIdx.x] = a;
        part_cnt[blockIdx.x] = k;
    }
}

__global__ __launch_bounds__(kFinalThreads) void finalize_kernel(const float *part_sum, const int *part_cnt, int nblk, Scalars *sc,
                                                                 float *loss, int *kept_out) {
    __shared__ double wsum[kFinalThreads / kWave];
    __shared__ int wcnt[kFinalThreads / kWave];
    double a = 0.0;
    int k = 0;
    for (int i = threadIdx.x; i < nblk; i += kFinalThreads) {
        a += part_sum[i];
        k += part_cnt[i];
    }
    a = wave_sum(a);
    k = wave_sum(k);
    if (lane_id() == 0) {
        wsum[threadIdx.x / kWave] = a;
        wcnt[threadIdx.x / kWave] = k;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        int n = 0;
        for (int w = 0; w < kFinalThreads / kWave; ++w) {
            s += wsum[w];
            n += wcnt[w];
        }
        sc->kept = n;
        *loss = (float)(s / (double)n);                 // 0 / 0 = NaN when nothing is kept, as F.cross_entropy
        if (kept_out) *kept_out = n;
    }
}

__global__ __launch_bounds__(kPixThreads) void backward_kernel(const float *grad_out, const float *logits, float *grad,
                                                               const float *pix_lse, const int *pix_tgt, const Scalars *sc,
                                                               int C, int HW, int N) {
    const int i = blockIdx.x * kPixThreads + threadIdx.x;
    if (i >= N) return;
    const int b = i / HW, r = i - b * HW;
    const size_t base = (size_t)b * C * HW + r;
    const int t = pix_tgt[i];
    if (t < 0) {
        for (int c = 0; c < C; ++c) grad[base + (size_t)c * HW] = 0.f;
        return;
    }
    const float scale = grad_out[0] / (float)sc->kept;
    const float lse = pix_lse[i];
    for (int c = 0; c < C; ++c) {
        const float p = expf(logits[base + (size_t)c * HW] - lse);
        grad[base + (size_t)c * HW] = (c == t ? p - 1.f : p) * scale;
    }
}

}  // namespace ohem
