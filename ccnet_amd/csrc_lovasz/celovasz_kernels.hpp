// celovasz_kernels.hpp -- the kernels behind include/ccnet_celovasz.h: cross-entropy + Lovász-softmax of low-resolution
// logits that are up-sampled (and soft-maxed) as they are read.
//
//   pixel_errors   one thread per full-resolution pixel, consecutive lanes along W: the pixel's footprint, the log-sum-exp of its
//                  C interpolated logits (dsn::pixel_head) and lse - z_target for the cross-entropy, then for every class
//                  p_c = prob(z_c, lse) and the sort key and payload of e = |fg - p_c| in the format of lovasz::errors_kernel
//                  (coalesced along the pixel index per class).  The log-sum-exp and the two-byte label go to the workspace,
//                  one (sum, valid, out-of-range) partial per block
//   sort, scan     lovasz::'s radix, scan and finalize passes, unchanged (lovasz_launch.hpp): g * (-sign) at every pixel's
//                  slot, seg_mult, seg_den, the Lovász mean
//   finalize       one workgroup: the cross-entropy partials summed in a fixed order (double), CE = sum / valid,
//                  loss = CE + LS, the scalars the backward reads
//   pixel_dot      one thread per pixel: s = sum_k p_k * G_k (G without grad_out), 4 bytes a pixel, so that no thread of the
//                  backward sums over the classes
//   backward       the gather of dsn::backward_kernel (same grid, 3 x 3 register patch, membership by dsn::axis_taps, fixed
//                  order; the threads numbered class-fastest as in ohemdsn::backward_kernel): per full-resolution pixel of
//                  the footprint (p_c - 1[t = c]) for the cross-entropy and p_c * (G_c - s) for the Lovász term
// The up-sample arithmetic (axis_taps, bilinear, candidates, pick3, pixel_head) is dsn::'s and the key format, sort and scan
// are lovasz::'s; neither is restated.  p_c has one definition, prob(), for the errors, for s and for the gradient.
#pragma once
#include "lovasz_kernels.hpp"

#include <dsn_kernels.hpp>

namespace celovasz {

using lovasz::kWave;
using lovasz::lane_id;
using lovasz::wave_sum;

constexpr int kPixThreads = 256;       // pixel_errors / pixel_dot / backward blocks
constexpr int kFinalThreads = 256;

struct Scalars {                       // device-side results of one forward, read by the backward
    int valid;
    int out_of_range;
    int n_kept;                        // written by lovasz::finalize_kernel
    float ls;                          // the Lovász mean, written by lovasz::finalize_kernel
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

// the softmax probability of a class with interpolated logit z at a pixel whose log-sum-exp is lse: the one definition of p_c
__device__ __forceinline__ float prob(float z, float lse) { return expf(z - lse); }

// d loss / d p_c = grad_out * coef * (g * (-sign)) for a pixel of segment s (rule 5 of ccnet_lovasz.h without grad_out)
__device__ __forceinline__ float class_coef(const int *seg_mult, const int *seg_den, size_t s, int B, int per_image) {
    const int m = seg_mult[s];
    return m ? (float)m * ((per_image ? 1.f / (float)B : 1.f) / (float)seg_den[s]) : 0.f;
}

__global__ __launch_bounds__(kPixThreads) void pixel_errors_kernel(const float *logits, const int64_t *target, uint32_t *keys,
                                                                   uint32_t *pays, float *part_sum, int *part_cnt,
                                                                   float *pix_lse, int16_t *pix_tgt, int C, int h, int w, int H,
                                                                   int W, int N, int L, int per_image, float sh, float sw,
                                                                   long long ignore) {
    __shared__ float wsum[kPixThreads / kWave];
    __shared__ int wcnt[2][kPixThreads / kWave];
    const int i = blockIdx.x * kPixThreads + threadIdx.x;
    float nll = 0.f;
    int valid = 0, oor = 0;
    if (i < N) {
        const int HW = H * W, b = i / HW, r = i - b * HW, oy = r / W, ox = r - oy * W;
        const long long lab = target[i];
        const bool in_range = lab >= 0 && lab < C;
        valid = lab != ignore && in_range;
        oor = lab != ignore && !in_range;
        const uint32_t idx = per_image ? (uint32_t)r : (uint32_t)i;              // the pixel's index in its segments
        const size_t seg0 = (per_image ? (size_t)b * C : (size_t)0) * (size_t)L + idx;
        float lse = 0.f;
        if (valid) {
            const int t = (int)lab, plane = h * w;
            const float *img = logits + (size_t)b * C * plane;
            const Foot f = footprint(sh, sw, oy, ox, h, w);
            float zt;
            dsn::pixel_head(img, C, plane, f.o00, f.o01, f.o10, f.o11, f.ty, f.tx, t, lse, zt);
            nll = lse - zt;
            for (int c = 0; c < C; ++c) {
                const float p = prob(logit_at(img + (size_t)c * plane, f), lse);
                const bool fg = c == t;
                const float d = (fg ? 1.f : 0.f) - p;
                const size_t at = seg0 + (size_t)c * L;
                keys[at] = lovasz::kKeyTop - lovasz::float_to_bits(fabsf(d));
                pays[at] = idx | (fg ? lovasz::kFgBit : 0u) | (d < 0.f ? lovasz::kUpBit : 0u) | (d > 0.f ? lovasz::kDownBit : 0u);
            }
        } else {
            // not valid: sorts last, g = 0 whatever the payload's flags say; only the index is read
            for (int c = 0; c < C; ++c) {
                const size_t at = seg0 + (size_t)c * L;
                keys[at] = lovasz::kInvalidKey;
                pays[at] = idx;
            }
        }
        pix_lse[i] = lse;
        pix_tgt[i] = valid ? (int16_t)lab : (int16_t)-1;
    }
    nll = wave_sum(nll);
    valid = wave_sum(valid);
    oor = wave_sum(oor);
    if (lane_id() == 0) {
        const int v = threadIdx.x / kWave;
        wsum[v] = nll;
        wcnt[0][v] = valid;
        wcnt[1][v] = oor;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f;
        int k0 = 0, k1 = 0;
        for (int v = 0; v < kPixThreads / kWave; ++v) {
            a += wsum[v];
            k0 += wcnt[0][v];
            k1 += wcnt[1][v];
        }
        part_sum[blockIdx.x] = a;
        part_cnt[2 * blockIdx.x] = k0;
        part_cnt[2 * blockIdx.x + 1] = k1;
    }
}

// after lovasz::finalize_kernel, which left the Lovász mean and the kept class count in `sc`
__global__ __launch_bounds__(kFinalThreads) void finalize_kernel(const float *part_sum, const int *part_cnt, int nblk, Scalars *sc,
                                                                 float *loss, float *head_loss, int *counts) {
    __shared__ double wsum[kFinalThreads / kWave];
    __shared__ int wcnt[2][kFinalThreads / kWave];
    double a = 0.0;
    int k0 = 0, k1 = 0;
    for (int i = threadIdx.x; i < nblk; i += kFinalThreads) {
        a += part_sum[i];
        k0 += part_cnt[2 * i];
        k1 += part_cnt[2 * i + 1];
    }
    a = wave_sum(a);
    k0 = wave_sum(k0);
    k1 = wave_sum(k1);
    if (lane_id() == 0) {
        const int v = threadIdx.x / kWave;
        wsum[v] = a;
        wcnt[0][v] = k0;
        wcnt[1][v] = k1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        int valid = 0, oor = 0;
        for (int v = 0; v < kFinalThreads / kWave; ++v) {
            s += wsum[v];
            valid += wcnt[0][v];
            oor += wcnt[1][v];
        }
        sc->valid = valid;
        sc->out_of_range = oor;
        const float ce = (float)(s / (double)valid);          // 0 / 0 = NaN when no pixel is valid, as F.cross_entropy
        const float ls = sc->ls;
        *loss = ce + ls;
        if (head_loss) {
            head_loss[0] = ce;
            head_loss[1] = ls;
        }
        if (counts) {
            counts[0] = valid;
            counts[1] = oor;
            counts[2] = sc->n_kept;
        }
    }
}

// grid (ceil(H * W / kPixThreads), B): s = sum_k p_k * coef_k * g_k at every pixel, 0 where the label is not valid
__global__ __launch_bounds__(kPixThreads) void pixel_dot_kernel(const float *logits, const float *gbuf, const int *seg_mult,
                                                                const int *seg_den, const float *pix_lse, const int16_t *pix_tgt,
                                                                float *pix_dot, int B, int C, int h, int w, int H, int W, int L,
                                                                int per_image, float sh, float sw) {
    __shared__ float coef[lovasz::kMaxClasses];
    const int b = blockIdx.y, HW = H * W;
    for (int c = threadIdx.x; c < C; c += kPixThreads)
        coef[c] = class_coef(seg_mult, seg_den, per_image ? (size_t)b * C + c : (size_t)c, B, per_image);
    __syncthreads();
    const int r = blockIdx.x * kPixThreads + threadIdx.x;
    if (r >= HW) return;
    const size_t i = (size_t)b * HW + r;
    float acc = 0.f;
    if (pix_tgt[i] >= 0) {
        const int oy = r / W, ox = r - oy * W, plane = h * w;
        const float *img = logits + (size_t)b * C * plane;
        const float *g = gbuf + (per_image ? (size_t)b * C * (size_t)L + r : i);
        const Foot f = footprint(sh, sw, oy, ox, h, w);
        const float lse = pix_lse[i];
        for (int c = 0; c < C; ++c)
            if (coef[c] != 0.f) acc += prob(logit_at(img + (size_t)c * plane, f), lse) * (coef[c] * g[(size_t)c * L]);
    }
    pix_dot[i] = acc;
}

// grid (ceil(h * w / kPixThreads), C, B), dsn::backward_kernel's; the threads of one image's slice of it are numbered with the
// class fastest (ohemdsn::backward_kernel says why): the label, the log-sum-exp and s of a step of the walk come from one or
// two cache lines a wave
__global__ __launch_bounds__(kPixThreads) void backward_kernel(const float *grad_out, const float *logits, float *grad,
                                                               const float *gbuf, const int *seg_mult, const int *seg_den,
                                                               const float *pix_lse, const int16_t *pix_tgt,
                                                               const float *pix_dot, const Scalars *sc, int B, int C, int h,
                                                               int w, int H, int W, int L, int per_image, float sh, float sw) {
    const unsigned lin = (blockIdx.y * gridDim.x + blockIdx.x) * kPixThreads + threadIdx.x;   // below C * (h * w + 255) < 2^32
    const int p = (int)(lin / (unsigned)C), c = (int)(lin - (unsigned)p * (unsigned)C);
    if (p >= h * w) return;
    const int b = blockIdx.z;
    const int y = p / w, x = p - y * w;
    const size_t at = ((size_t)b * C + c) * (size_t)(h * w);
    const float *img = logits + at;
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
    const size_t pix0 = (size_t)b * H * W;
    const float *lse = pix_lse + pix0, *dot = pix_dot + pix0;
    const int16_t *tgt = pix_tgt + pix0;
    const size_t seg = per_image ? (size_t)b * C + c : (size_t)c;
    const float *g = gbuf + seg * (size_t)L + (per_image ? (size_t)0 : pix0);
    const float coef = class_coef(seg_mult, seg_den, seg, B, per_image);
    int ylo, yhi, xlo, xhi;
    dsn::candidates(y, h, H, ylo, yhi);
    dsn::candidates(x, w, W, xlo, xhi);
    float acc_ce = 0.f, acc_ls = 0.f;
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
        float row_ce = 0.f, row_ls = 0.f;
        for (int ox = xlo; ox <= xhi; ++ox) {
            const dsn::Taps tx = dsn::axis_taps(sw, ox, w);
            if (tx.i0 != x && tx.i1 != x) continue;
            const int o = oy * W + ox;
            const int t = tgt[o];
            if (t < 0) continue;
            const float wx = (tx.i0 == x ? tx.l0 : 0.f) + (tx.i1 == x ? tx.l1 : 0.f);
            const int s0 = tx.i0 - (x - 1), s1 = tx.i1 - (x - 1);
            const float z = dsn::bilinear(ty, tx, dsn::pick3(top, s0), dsn::pick3(top, s1), dsn::pick3(bot, s0), dsn::pick3(bot, s1));
            const float pc = prob(z, lse[o]);
            row_ce += wx * (t == c ? pc - 1.f : pc);
            row_ls += wx * (pc * (coef * g[o] - dot[o]));
        }
        acc_ce += wy * row_ce;
        acc_ls += wy * row_ls;
    }
    const int n = sc->valid;
    const float go = grad_out[0];
    grad[at + p] = n > 0 ? go * (acc_ce / (float)n) + go * acc_ls : 0.f;     // nothing valid: zero, not 0 * inf
}

}  // namespace celovasz
