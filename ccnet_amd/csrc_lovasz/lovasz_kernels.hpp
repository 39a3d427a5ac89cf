// lovasz_kernels.hpp -- the kernels behind include/ccnet_lovasz.h.
//
// A segment is one class over one image (per_image) or over the batch; its L pixels are cut into tiles of kTile sorted
// positions, and every sort and scan launch runs a (tile, segment) grid, so all segments of a call sort at once.
//
//   errors          one thread per pixel, coalesced along W: e = |fg - p_c| for every class, written as a descending sort
//                   key (kKeyTop - bits(e); kInvalidKey, which sorts last, for pixels that are not valid) and a payload
//                   (pixel index in the segment | fg bit | the sign of d e / d p)
//   radix_hist      \
//   radix_offsets    > x 4 (8-bit digits, least significant first): a stable segmented LSD radix sort.  Per-tile digit
//   radix_scatter   /  histograms; their exclusive scan in (digit, tile) order per segment; a stable scatter ranked with
//                      ballots inside the wave, staged through LDS so each digit's run leaves the tile contiguously
//   scan_count      per tile: fg count and valid count of the sorted positions
//   scan_offsets    per segment: exclusive scan of the tile fg counts; gts and the valid count
//   scan_grad       per tile: inclusive fg prefix (ballot + LDS), J and g at every valid position with exact integer counts,
//                   g * (-sign) scattered to the pixel's slot, one fixed-order partial of sum e * g (double)
//   finalize        one workgroup: the partials summed per segment in a fixed order (double), the kept classes, the means
//   backward        one thread per pixel: grad = weight * ((grad_out [/ B] / n_kept) * g * (-sign)), written once
// Nothing waits on another workgroup inside a launch: every cross-tile dependency is a launch boundary.
#pragma once
#include <lovasz_platform.hpp>

#include <math.h>
#include <stdint.h>
#include <string.h>

namespace lovasz {

constexpr int kThreads = 256;                  // every launch but finalize's single workgroup uses this block
constexpr int kItems = 8;                      // sorted positions per thread and tile
constexpr int kTile = kThreads * kItems;       // positions per tile
constexpr int kRadix = 256;                    // 8-bit digits
constexpr int kMaxClasses = 256;
constexpr uint32_t kKeyTop = 0x7fffffffu;      // key = kKeyTop - bits(e): larger errors sort first, all keys <= kKeyTop
constexpr uint32_t kInvalidKey = 0xffffffffu;  // pixels that are not valid sort after every valid one
constexpr uint32_t kFgBit = 1u << 31;
constexpr uint32_t kUpBit = 1u << 30;          // d e / d p = +1 (fg - p < 0)
constexpr uint32_t kDownBit = 1u << 29;        // d e / d p = -1 (fg - p > 0)
constexpr uint32_t kIndexMask = (1u << 24) - 1;
constexpr int kMaxSegment = 1 << 24;

static_assert(kThreads == kRadix, "one thread per digit in the histogram and offset kernels");

struct ClassSel {                              // the class selection, passed by value in the kernel arguments
    unsigned char weight[kMaxClasses];         // multiplicity of every class (0: not selected)
    int present_only;                          // drop classes without a fg pixel in the segment
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

// exclusive scan of one value per thread over a 256-thread block (Hillis-Steele in `buf`); on return buf holds the inclusive
// scan, and every thread has passed the last barrier
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned *buf) {
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const unsigned add = tid >= off ? buf[tid - off] : 0u;
        __syncthreads();
        buf[tid] += add;
        __syncthreads();
    }
    return buf[tid] - v;
}

// J at a sorted position with `cf` fg and `cb` background pixels up to and including it (lovasz_grad's fp32 arithmetic)
__device__ __forceinline__ float jaccard(unsigned gts, unsigned cf, unsigned cb) {
    return 1.f - (float)(gts - cf) / (float)(gts + cb);
}

__global__ __launch_bounds__(kThreads) void errors_kernel(const float *probas, const int64_t *labels, uint32_t *keys,
                                                          uint32_t *pays, int C, int HW, int L, long long ignore,
                                                          int ignore_none, int per_image) {
    const int b = blockIdx.y;
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= HW) return;
    const long long lab = labels[(size_t)b * HW + r];
    const bool valid = ignore_none || lab != ignore;
    const uint32_t i = per_image ? (uint32_t)r : (uint32_t)b * (uint32_t)HW + (uint32_t)r;
    const float *px = probas + (size_t)b * C * HW + r;
    for (int c = 0; c < C; ++c) {
        const float p = px[(size_t)c * HW];
        const bool fg = valid && lab == c;
        const float d = (fg ? 1.f : 0.f) - p;
        const size_t at = (per_image ? (size_t)b * C + c : (size_t)c) * (size_t)L + i;
        keys[at] = valid ? kKeyTop - float_to_bits(fabsf(d)) : kInvalidKey;
        pays[at] = i | (fg ? kFgBit : 0u) | (d < 0.f ? kUpBit : 0u) | (d > 0.f ? kDownBit : 0u);
    }
}

__global__ __launch_bounds__(kThreads) void radix_hist_kernel(const uint32_t *keys, unsigned *counts, int L, int nt,
                                                              int shift) {
    __shared__ unsigned hist[kRadix];
    const int t = blockIdx.x;
    const size_t s = blockIdx.y;
    hist[threadIdx.x] = 0;
    __syncthreads();
    const int n = imin(kTile, L - t * kTile);
    const uint32_t *k = keys + s * (size_t)L + (size_t)t * kTile;
    for (int j = threadIdx.x; j < n; j += kThreads) lds_inc(&hist[(k[j] >> shift) & 255u]);
    __syncthreads();
    counts[(s * nt + t) * kRadix + threadIdx.x] = hist[threadIdx.x];
}

// counts (segment, tile, digit) -> the segment-relative output offset of the tile's first key of that digit
__global__ __launch_bounds__(kThreads) void radix_offsets_kernel(unsigned *counts, int nt) {
    __shared__ unsigned buf[kRadix];
    unsigned *row = counts + (size_t)blockIdx.x * nt * kRadix + threadIdx.x;
    unsigned sum = 0;
    for (int t = 0; t < nt; ++t) sum += row[(size_t)t * kRadix];
    unsigned run = block_exclusive_scan(sum, buf);
    for (int t = 0; t < nt; ++t) {
        const unsigned c = row[(size_t)t * kRadix];
        row[(size_t)t * kRadix] = run;
        run += c;
    }
}

__global__ __launch_bounds__(kThreads) void radix_scatter_kernel(const uint32_t *kin, const uint32_t *pin, uint32_t *kout,
                                                                 uint32_t *pout, const unsigned *offsets, int L, int nt,
                                                                 int shift) {
    constexpr int kWaves = kThreads / kWave;
    __shared__ uint32_t s_key[kTile];
    __shared__ uint32_t s_pay[kTile];
    __shared__ unsigned s_cnt[kRadix];          // keys of each digit ranked so far (the tile histogram at the end)
    __shared__ unsigned s_incl[kRadix];         // inclusive scan of the tile histogram
    __shared__ unsigned s_base[kRadix];         // segment-relative output offset of the tile's digit runs
    __shared__ unsigned s_wave[kWaves][kRadix]; // keys of each digit per wave in the current round
    const int tid = threadIdx.x, w = tid / kWave;
    const int t = blockIdx.x;
    const size_t seg = (size_t)blockIdx.y * L;
    const int n = imin(kTile, L - t * kTile);
    const uint32_t *ki = kin + seg + (size_t)t * kTile;
    const uint32_t *pi = pin + seg + (size_t)t * kTile;
    s_cnt[tid] = 0;
    for (int q = 0; q < kWaves; ++q) s_wave[q][tid] = 0;
    s_base[tid] = offsets[((size_t)blockIdx.y * nt + t) * kRadix + tid];
    uint32_t key[kItems], pay[kItems];
    unsigned rank[kItems];
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const int j = it * kThreads + tid;
        key[it] = j < n ? ki[j] : 0u;
        pay[it] = j < n ? pi[j] : 0u;
        rank[it] = 0;
    }
    __syncthreads();
    // rounds in tile order (position it * kThreads + tid), lanes in lane order: the rank within a digit is stable
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const bool ok = it * kThreads + tid < n;
        const unsigned d = (key[it] >> shift) & 255u;
        uint64_t same = ballot(ok);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (d >> bit) & 1u;
            const uint64_t m = ballot(on);
            same &= on ? m : ~m;
        }
        const unsigned below = rank_below(same);
        if (ok && below == 0) s_wave[w][d] = popc64(same);
        __syncthreads();
        if (ok) {
            unsigned r = s_cnt[d] + below;
            for (int q = 0; q < w; ++q) r += s_wave[q][d];
            rank[it] = r;
        }
        __syncthreads();
        unsigned add = 0;
        for (int q = 0; q < kWaves; ++q) {
            add += s_wave[q][tid];
            s_wave[q][tid] = 0;
        }
        s_cnt[tid] += add;
        __syncthreads();
    }
    block_exclusive_scan(s_cnt[tid], s_incl);
    // local sort of the tile in LDS, then each digit's run goes out contiguously
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        if (it * kThreads + tid < n) {
            const unsigned d = (key[it] >> shift) & 255u;
            const unsigned pos = s_incl[d] - s_cnt[d] + rank[it];
            s_key[pos] = key[it];
            s_pay[pos] = pay[it];
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
        const int j = it * kThreads + tid;
        if (j < n) {
            const uint32_t k = s_key[j];
            const unsigned d = (k >> shift) & 255u;
            const size_t o = seg + s_base[d] + ((unsigned)j - (s_incl[d] - s_cnt[d]));
            kout[o] = k;
            pout[o] = s_pay[j];
        }
    }
}

__global__ __launch_bounds__(kThreads) void scan_count_kernel(const uint32_t *keys, const uint32_t *pays, unsigned *blk_fg,
                                                              unsigned *blk_valid, int L, int nt) {
    constexpr int kWaves = kThreads / kWave;
    __shared__ unsigned wf[kWaves], wv[kWaves];
    const int tid = threadIdx.x, w = tid / kWave;
    const int t = blockIdx.x;
    const size_t s = blockIdx.y;
    const int n = imin(kTile, L - t * kTile);
    const size_t base = s * (size_t)L + (size_t)t * kTile;
    unsigned f = 0, v = 0;
    for (int it = 0; it < kItems; ++it) {
        const int j = it * kThreads + tid;
        const bool ok = j < n;
        f += popc64(ballot(ok && (pays[base + (ok ? j : 0)] & kFgBit)));
        v += popc64(ballot(ok && keys[base + (ok ? j : 0)] != kInvalidKey));
    }
    if (lane_id() == 0) {
        wf[w] = f;
        wv[w] = v;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned a = 0, c = 0;
        for (int q = 0; q < kWaves; ++q) {
            a += wf[q];
            c += wv[q];
        }
        blk_fg[s * nt + t] = a;
        blk_valid[s * nt + t] = c;
    }
}

// one workgroup per segment: blk_fg becomes the fg count before each tile; gts and the valid count of the segment
__global__ __launch_bounds__(kThreads) void scan_offsets_kernel(unsigned *blk_fg, const unsigned *blk_valid, unsigned *seg_gts,
                                                                unsigned *seg_nvalid, int nt) {
    __shared__ unsigned buf_f[kThreads], buf_v[kThreads];
    const int tid = threadIdx.x;
    const size_t s = blockIdx.x;
    unsigned *f = blk_fg + s * nt;
    const unsigned *v = blk_valid + s * nt;
    const int per = (nt + kThreads - 1) / kThreads;
    const int t0 = imin(nt, tid * per), t1 = imin(nt, t0 + per);
    unsigned sf = 0, sv = 0;
    for (int t = t0; t < t1; ++t) {
        sf += f[t];
        sv += v[t];
    }
    const unsigned ef = block_exclusive_scan(sf, buf_f);
    const unsigned ev = block_exclusive_scan(sv, buf_v);
    unsigned run = ef;
    for (int t = t0; t < t1; ++t) {
        const unsigned c = f[t];
        f[t] = run;
        run += c;
    }
    if (tid == kThreads - 1) {
        seg_gts[s] = ef + sf;
        seg_nvalid[s] = ev + sv;
    }
}

__global__ __launch_bounds__(kThreads) void scan_grad_kernel(const uint32_t *keys, const uint32_t *pays,
                                                             const unsigned *blk_fg_off, const unsigned *seg_gts,
                                                             const unsigned *seg_nvalid, float *gbuf, double *blk_loss,
                                                             int L, int nt) {
    constexpr int kWaves = kThreads / kWave;
    __shared__ unsigned s_wave[kWaves];
    __shared__ double s_part[kWaves];
    const int tid = threadIdx.x, w = tid / kWave;
    const int t = blockIdx.x;
    const size_t s = blockIdx.y;
    const int n = imin(kTile, L - t * kTile);
    const size_t seg = s * (size_t)L;
    const size_t base = seg + (size_t)t * kTile;
    const unsigned gts = seg_gts[s], nvalid = seg_nvalid[s];
    unsigned run = blk_fg_off[s * nt + t];       // fg positions before this round
    double acc = 0.0;
    for (int it = 0; it < kItems; ++it) {
        const int j = it * kThreads + tid;
        const bool ok = j < n;
        const uint32_t key = ok ? keys[base + j] : kInvalidKey;
        const uint32_t pay = ok ? pays[base + j] : 0u;
        const unsigned fg = pay >> 31;
        const uint64_t m = ballot(fg != 0);
        if (lane_id() == 0) s_wave[w] = popc64(m);
        __syncthreads();
        unsigned before = run + rank_below(m), total = 0;
        for (int q = 0; q < kWaves; ++q) {
            if (q < w) before += s_wave[q];
            total += s_wave[q];
        }
        __syncthreads();
        run += total;
        if (ok) {
            const unsigned pos = (unsigned)(t * kTile + j);
            float gv = 0.f;
            if (pos < nvalid) {
                const unsigned cf = before + fg;                 // inclusive prefix counts, exact integers
                float g = jaccard(gts, cf, pos + 1 - cf);
                if (pos > 0) g -= jaccard(gts, cf - fg, pos - (cf - fg));
                acc += (double)bits_to_float(kKeyTop - key) * (double)g;
                gv = (pay & kUpBit) ? g : (pay & kDownBit) ? -g : 0.f;
            }
            gbuf[seg + (pay & kIndexMask)] = gv;
        }
    }
    acc = wave_sum(acc);
    if (lane_id() == 0) s_part[w] = acc;
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
        for (int q = 0; q < kWaves; ++q) a += s_part[q];
        blk_loss[s * nt + t] = a;
    }
}

__global__ __launch_bounds__(kThreads) void finalize_kernel(const double *blk_loss, const unsigned *seg_gts,
                                                            const unsigned *seg_nvalid, double *seg_loss, int *seg_mult,
                                                            int *seg_den, int nt, int B, int C, int per_image, ClassSel sel,
                                                            float *loss, int *n_kept_out) {
    const int S = per_image ? B * C : C;
    for (int s = threadIdx.x; s < S; s += kThreads) {
        double a = 0.0;
        for (int t = 0; t < nt; ++t) a += blk_loss[(size_t)s * nt + t];
        seg_loss[s] = a;
        const bool keep = seg_nvalid[s] > 0 && !(sel.present_only && seg_gts[s] == 0);
        seg_mult[s] = keep ? sel.weight[s % C] : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nimg = per_image ? B : 1;
        double total = 0.0;
        int kept = 0;
        for (int b = 0; b < nimg; ++b) {
            int den = 0;
            double num = 0.0;
            for (int c = 0; c < C; ++c) {
                den += seg_mult[b * C + c];
                num += seg_mult[b * C + c] * seg_loss[b * C + c];
            }
            for (int c = 0; c < C; ++c) seg_den[b * C + c] = den;
            if (den) total += num / den;
            kept += den;
        }
        *loss = (float)(total / nimg);
        if (n_kept_out) *n_kept_out = kept;
    }
}

__global__ __launch_bounds__(kThreads) void backward_kernel(const float *grad_out, float *grad, const float *gbuf,
                                                            const int *seg_mult, const int *seg_den, int B, int C, int HW,
                                                            int L, int per_image) {
    __shared__ float fac[kMaxClasses], mult[kMaxClasses];
    const int b = blockIdx.y;
    if ((int)threadIdx.x < C) {
        const size_t s = per_image ? (size_t)b * C + threadIdx.x : threadIdx.x;
        const int m = seg_mult[s];
        float t = grad_out[0];
        if (per_image) t = t / (float)B;
        fac[threadIdx.x] = m ? t / (float)seg_den[s] : 0.f;
        mult[threadIdx.x] = (float)m;
    }
    __syncthreads();
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= HW) return;
    const size_t i = per_image ? (size_t)r : (size_t)b * HW + r;
    float *out = grad + (size_t)b * C * HW + r;
    for (int c = 0; c < C; ++c) {
        const size_t s = per_image ? (size_t)b * C + c : (size_t)c;
        out[(size_t)c * HW] = mult[c] != 0.f ? mult[c] * (fac[c] * gbuf[s * L + i]) : 0.f;
    }
}

}  // namespace lovasz
