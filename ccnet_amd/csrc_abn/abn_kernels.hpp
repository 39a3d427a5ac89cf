// abn_kernels.hpp -- the kernels behind include/ccnet_abn.h.
//
// Two partitions of an NCHW tensor:
//   reduction    workgroup (c, s) of a C x S grid takes the slice [s chunk, (s + 1) chunk) of channel c's N * H * W elements
//                in (n, h, w) order and writes one fp64 partial pair; a finalize kernel (one thread per channel) adds the S
//                pairs in split order.  S depends on the shape only, so every sum has one fixed order.
//   elementwise  workgroup (plane, chunk) takes kBlockElems consecutive elements of one (n, c) plane.
// Inside a workgroup every thread walks 16-byte groups of the flat tensor (4 fp32 or 8 bf16 elements): a group that lies
// wholly inside the workgroup's range is one vector load or store (when the caller's pointers are 16-byte aligned), a group
// cut by the range -- planes of odd H * W start anywhere -- is handled element by element, so neighbouring workgroups never
// write the same element.  Each thread issues all loads of a batch before its first store: with y aliasing x (in place) an
// element is read and written by the same thread only.
//
//   stats_partial     shifted sums s1 = sum (x - K), s2 = sum (x - K)^2 in fp64, K = the channel's first element
//   stats_finalize    (count, mean = K + s1 / n, M2 = s2 - s1^2 / n) per channel
//   stats_combine     Chan's merge of R ranks' triples in rank order; saved = (mean, invstd, n); running statistics
//   forward           y = act(gamma (x - mean) invstd + beta [+ residual])
//   backward_partial  dz = dy act'(y), xhat from x or from y; fp64 partials of sum dz and sum dz xhat
//   backward_finalize per channel: the local sums, dweight, dbias
//   backward_apply    dx = gamma invstd (dz - sum dz / n - xhat sum dz xhat / n) (eval: gamma invstd dz); dresidual = dz
// Nothing is accumulated through memory and no workgroup waits on another: every cross-workgroup dependency is a launch
// boundary.
#pragma once
#include <abn_platform.hpp>

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace abn {

constexpr int kThreads = 256;                       // every launch uses this block
constexpr int kPerThread = 16;                      // elements per thread and batch: 4 fp32 or 2 bf16 groups
constexpr int kBlockElems = kThreads * kPerThread;  // elements of one elementwise workgroup
constexpr int kTargetBlocks = 2048;                 // reduction launches aim at about 8 workgroups per CU ...
constexpr long long kMinSplit = 8192;               // ... of at least this many elements each

enum { kIdentity = 0, kRelu = 1, kLeaky = 2, kElu = 3 };
enum { kFromInput = 0, kFromOutput = 1 };

struct Op {
    int act;
    float p;          // leaky slope / elu alpha
    int abs_eps;      // gamma = |weight| + eps
    float eps;
};

__device__ __forceinline__ float bf16_bits_to_float(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
__device__ __forceinline__ uint16_t float_to_bf16_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);   // a NaN stays a quiet NaN
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                    // round to nearest even
}

template <class T>
struct Elem;
template <>
struct Elem<float> {
    static constexpr int V = 4;
    __device__ static float get(const float *p, size_t i) { return p[i]; }
    __device__ static void put(float *p, size_t i, float v) { p[i] = v; }
    __device__ static void getv(const float *p, size_t i, float (&o)[V]) {
        const uint4 q = load16(p + i);
        memcpy(o, &q, 16);
    }
    __device__ static void putv(float *p, size_t i, const float (&v)[V]) {
        uint4 q;
        memcpy(&q, v, 16);
        store16(p + i, q);
    }
};
template <>
struct Elem<uint16_t> {                             // bf16 as its bit pattern
    static constexpr int V = 8;
    __device__ static float get(const uint16_t *p, size_t i) { return bf16_bits_to_float(p[i]); }
    __device__ static void put(uint16_t *p, size_t i, float v) { p[i] = float_to_bf16_bits(v); }
    __device__ static void getv(const uint16_t *p, size_t i, float (&o)[V]) {
        const uint4 q = load16(p + i);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[2 * k] = bf16_bits_to_float((uint16_t)(w[k] & 0xffffu));
            o[2 * k + 1] = bf16_bits_to_float((uint16_t)(w[k] >> 16));
        }
    }
    __device__ static void putv(uint16_t *p, size_t i, const float (&v)[V]) {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            w[k] = (uint32_t)float_to_bf16_bits(v[2 * k]) | ((uint32_t)float_to_bf16_bits(v[2 * k + 1]) << 16);
        uint4 q;
        q.x = w[0];
        q.y = w[1];
        q.z = w[2];
        q.w = w[3];
        store16(p + i, q);
    }
};

// group g = elements [g V, g V + V) of the flat tensor; `full`: the whole group lies in [f0, f1) and may be one vector access
template <class T>
__device__ __forceinline__ void load_group(const T *p, size_t g, size_t f0, size_t f1, bool full,
                                           float (&o)[Elem<T>::V]) {
    constexpr int V = Elem<T>::V;
    if (full) {
        Elem<T>::getv(p, g * V, o);
        return;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const size_t i = g * V + e;
        o[e] = (i >= f0 && i < f1) ? Elem<T>::get(p, i) : 0.f;
    }
}
template <class T>
__device__ __forceinline__ void store_group(T *p, size_t g, size_t f0, size_t f1, bool full,
                                            const float (&v)[Elem<T>::V]) {
    constexpr int V = Elem<T>::V;
    if (full) {
        Elem<T>::putv(p, g * V, v);
        return;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const size_t i = g * V + e;
        if (i >= f0 && i < f1) Elem<T>::put(p, i, v[e]);
    }
}

__device__ __forceinline__ float act_forward(float z, int act, float p) {
    switch (act) {
        case kRelu: return z > 0.f ? z : 0.f;
        case kLeaky: return z > 0.f ? z : z * p;
        case kElu: return z > 0.f ? z : p * expm1f(z);
        default: return z;
    }
}
// d act / dz from the output y
__device__ __forceinline__ float act_grad(float y, int act, float p) {
    switch (act) {
        case kRelu: return y > 0.f ? 1.f : 0.f;
        case kLeaky: return y > 0.f ? 1.f : p;
        case kElu: return y > 0.f ? 1.f : y + p;
        default: return 1.f;
    }
}
// z from y (identity, leaky p > 0, elu)
__device__ __forceinline__ float act_inverse(float y, int act, float p) {
    if (y > 0.f) return y;
    if (act == kLeaky) return y / p;
    if (act == kElu) return log1pf(fmaxf(y / p, -1.f + 0x1p-24f));
    return y;
}

struct Chan {
    float mean, invstd, gamma, beta;
};

// the channel's statistics (saved: training; NULL: the running ones) and affine step
__device__ __forceinline__ Chan channel(int c, int C, const double *saved, const float *rm, const float *rv, const float *w,
                                        const float *b, const Op &op) {
    Chan k;
    if (saved) {
        k.mean = (float)saved[c];
        k.invstd = (float)saved[C + c];
    } else {
        k.mean = rm[c];
        k.invstd = 1.f / sqrtf(rv[c] + op.eps);
    }
    const float g = w ? w[c] : 1.f;
    k.gamma = op.abs_eps ? fabsf(g) + op.eps : g;
    k.beta = b ? b[c] : 0.f;
    return k;
}

// (a, b) summed over the block in a fixed order: the wave butterfly, then the waves in index order
__device__ __forceinline__ void block_sum2(double &a, double &b) {
    __shared__ double red[2][kThreads / kWave];
    a = wave_sum(a);
    b = wave_sum(b);
    const int w = threadIdx.x / kWave;
    if (lane_id() == 0) {
        red[0][w] = a;
        red[1][w] = b;
    }
    __syncthreads();
    a = red[0][0];
    b = red[1][0];
#pragma unroll
    for (int i = 1; i < kThreads / kWave; ++i) {
        a += red[0][i];
        b += red[1][i];
    }
}

// the flat range [f0, f1) of plane n of channel c that reduction workgroup (c, s) covers
struct Slice {
    size_t f0, f1;
};
__device__ __forceinline__ Slice plane_slice(long long n, int c, int C, int HW, long long m0, long long m1) {
    const long long p0 = n * HW;
    const size_t base = ((size_t)n * C + c) * (size_t)HW;
    return {base + (size_t)((m0 > p0 ? m0 : p0) - p0), base + (size_t)((m1 < p0 + HW ? m1 : p0 + HW) - p0)};
}

template <class T>
__global__ __launch_bounds__(kThreads) void stats_partial_kernel(const T *x, double *part, int N, int C, int HW, int S,
                                                                 long long chunk, int vec) {
    constexpr int V = Elem<T>::V, U = kPerThread / V;
    const int c = blockIdx.x / S, s = blockIdx.x % S;
    const long long M = (long long)N * HW, m0 = s * chunk, m1 = m0 + chunk < M ? m0 + chunk : M;
    const float K = Elem<T>::get(x, (size_t)c * HW);
    double s1 = 0.0, s2 = 0.0;
    for (long long n = m0 / HW; n * HW < m1; ++n) {
        const Slice r = plane_slice(n, c, C, HW, m0, m1);
        const size_t g1 = (r.f1 + V - 1) / V;
        for (size_t gb = r.f0 / V + threadIdx.x; gb < g1; gb += (size_t)kThreads * U) {
            float v[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t g = gb + (size_t)u * kThreads;
                if (g < g1) load_group(x, g, r.f0, r.f1, vec && g * V >= r.f0 && g * V + V <= r.f1, v[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t g = gb + (size_t)u * kThreads;
                if (g >= g1) continue;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const size_t i = g * V + e;
                    if (i < r.f0 || i >= r.f1) continue;
                    const double d = (double)(v[u][e] - K);
                    s1 += d;
                    s2 = fma(d, d, s2);
                }
            }
        }
    }
    block_sum2(s1, s2);
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = s1;
        part[2 * (size_t)blockIdx.x + 1] = s2;
    }
}

template <class T>
__global__ __launch_bounds__(kThreads) void stats_finalize_kernel(const T *x, const double *part, double *local, int N,
                                                                  int C, int HW, int S) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < S; ++s) {
        s1 += part[2 * ((size_t)c * S + s)];
        s2 += part[2 * ((size_t)c * S + s) + 1];
    }
    const double n = (double)N * (double)HW, dm = s1 / n;
    local[c] = n;
    local[C + c] = (double)Elem<T>::get(x, (size_t)c * HW) + dm;
    const double m2 = s2 - s1 * dm;
    local[2 * C + c] = m2 < 0.0 ? 0.0 : m2;          // clamps negative rounding residue; a NaN stays (fmax would return 0)
}

__global__ __launch_bounds__(kThreads) void stats_combine_kernel(const double *all, int R, int C, float eps, float momentum,
                                                                 float *rm, float *rv, double *saved) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    double n = all[c], mean = all[C + c], m2 = all[2 * C + c];
    for (int r = 1; r < R; ++r) {
        const double *a = all + (size_t)r * 3 * C;
        const double nb = a[c], nab = n + nb, delta = a[C + c] - mean;
        mean += delta * (nb / nab);
        m2 += a[2 * C + c] + delta * delta * (n * nb / nab);
        n = nab;
    }
    const double var = m2 / n, m = (double)momentum;
    saved[c] = mean;
    saved[C + c] = 1.0 / sqrt(var + (double)eps);
    saved[2 * C + c] = n;
    if (rm) rm[c] = (float)((1.0 - m) * (double)rm[c] + m * mean);
    if (rv) rv[c] = (float)((1.0 - m) * (double)rv[c] + m * (m2 / (n - 1.0)));
}

template <class T>
__global__ __launch_bounds__(kThreads) void forward_kernel(const T *x, const T *res, T *y, const double *saved,
                                                           const float *rm, const float *rv, const float *w, const float *b,
                                                           int C, int HW, int cpp, Op op, int vec) {
    constexpr int V = Elem<T>::V, U = kPerThread / V;
    const size_t plane = blockIdx.x / cpp;
    const int chunk = blockIdx.x % cpp, c = (int)(plane % C);
    const Chan k = channel(c, C, saved, rm, rv, w, b, op);
    const float scale = k.gamma * k.invstd;
    const size_t base = plane * HW, f0 = base + (size_t)chunk * kBlockElems;
    const size_t f1 = base + ((size_t)(chunk + 1) * kBlockElems < (size_t)HW ? (size_t)(chunk + 1) * kBlockElems : HW);
    const size_t g1 = (f1 + V - 1) / V;
    for (size_t gb = f0 / V + threadIdx.x; gb < g1; gb += (size_t)kThreads * U) {
        float v[U][V], r[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t g = gb + (size_t)u * kThreads;
            if (g >= g1) continue;
            const bool full = vec && g * V >= f0 && g * V + V <= f1;
            load_group(x, g, f0, f1, full, v[u]);
            if (res) load_group(res, g, f0, f1, full, r[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t g = gb + (size_t)u * kThreads;
            if (g >= g1) continue;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float z = (v[u][e] - k.mean) * scale + k.beta;
                if (res) z += r[u][e];
                v[u][e] = act_forward(z, op.act, op.p);
            }
            store_group(y, g, f0, f1, vec && g * V >= f0 && g * V + V <= f1, v[u]);
        }
    }
}

// dz and xhat of one element: s is x (kFromInput) or y (kFromOutput), yv is y for act' (kFromInput), r the residual
__device__ __forceinline__ void dz_xhat(int source, const Op &op, const Chan &k, float inv_gamma, float s, float yv, float dyv,
                                        float r, float &dz, float &xhat) {
    if (source == kFromInput) {
        xhat = (s - k.mean) * k.invstd;
        dz = dyv * act_grad(yv, op.act, op.p);
    } else {
        xhat = (act_inverse(s, op.act, op.p) - k.beta - r) * inv_gamma;
        dz = dyv * act_grad(s, op.act, op.p);
    }
}

template <class T>
__global__ __launch_bounds__(kThreads) void backward_partial_kernel(const T *src, const T *y, const T *dy, const T *res,
                                                                    const double *saved, const float *rm, const float *rv,
                                                                    const float *w, const float *b, double *part, int N,
                                                                    int C, int HW, int S, long long chunk, Op op,
                                                                    int source, int vec) {
    constexpr int V = Elem<T>::V, U = kPerThread / V;
    const int c = blockIdx.x / S, s = blockIdx.x % S;
    const long long M = (long long)N * HW, m0 = s * chunk, m1 = m0 + chunk < M ? m0 + chunk : M;
    const Chan k = channel(c, C, saved, rm, rv, w, b, op);
    const float inv_gamma = 1.f / k.gamma;
    const bool need_y = source == kFromInput && op.act != kIdentity;
    const bool need_r = source == kFromOutput && res != nullptr;
    double s1 = 0.0, s2 = 0.0;
    for (long long n = m0 / HW; n * HW < m1; ++n) {
        const Slice sl = plane_slice(n, c, C, HW, m0, m1);
        const size_t g1 = (sl.f1 + V - 1) / V;
        for (size_t gb = sl.f0 / V + threadIdx.x; gb < g1; gb += (size_t)kThreads * U) {
            float vs[U][V], vy[U][V], vd[U][V], vr[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t g = gb + (size_t)u * kThreads;
                if (g >= g1) continue;
                const bool full = vec && g * V >= sl.f0 && g * V + V <= sl.f1;
                load_group(src, g, sl.f0, sl.f1, full, vs[u]);
                load_group(dy, g, sl.f0, sl.f1, full, vd[u]);
                if (need_y) load_group(y, g, sl.f0, sl.f1, full, vy[u]);
                if (need_r) load_group(res, g, sl.f0, sl.f1, full, vr[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t g = gb + (size_t)u * kThreads;
                if (g >= g1) continue;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const size_t i = g * V + e;
                    if (i < sl.f0 || i >= sl.f1) continue;
                    float dz, xhat;
                    dz_xhat(source, op, k, inv_gamma, vs[u][e], need_y ? vy[u][e] : 0.f, vd[u][e], need_r ? vr[u][e] : 0.f,
                            dz, xhat);
                    s1 += (double)dz;
                    s2 = fma((double)dz, (double)xhat, s2);
                }
            }
        }
    }
    block_sum2(s1, s2);
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = s1;
        part[2 * (size_t)blockIdx.x + 1] = s2;
    }
}

__global__ __launch_bounds__(kThreads) void backward_finalize_kernel(const double *part, const float *w, double *sums,
                                                                     float *dweight, float *dbias, int C, int S,
                                                                     int abs_eps) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < S; ++s) {
        s1 += part[2 * ((size_t)c * S + s)];
        s2 += part[2 * ((size_t)c * S + s) + 1];
    }
    sums[c] = s1;
    sums[C + c] = s2;
    if (dbias) dbias[c] = (float)s1;
    if (dweight) {
        const float g = w ? w[c] : 1.f;
        const double sign = !abs_eps ? 1.0 : g > 0.f ? 1.0 : g < 0.f ? -1.0 : 0.0;
        dweight[c] = (float)(s2 * sign);
    }
}

template <class T>
__global__ __launch_bounds__(kThreads) void backward_apply_kernel(const T *src, const T *y, const T *dy, const T *res,
                                                                  const double *saved, const float *rm, const float *rv,
                                                                  const float *w, const float *b, const double *all_sums,
                                                                  int R, T *dx, T *dres, int C, int HW, int cpp, Op op,
                                                                  int source, int vec) {
    constexpr int V = Elem<T>::V, U = kPerThread / V;
    const size_t plane = blockIdx.x / cpp;
    const int chunk = blockIdx.x % cpp, c = (int)(plane % C);
    const Chan k = channel(c, C, saved, rm, rv, w, b, op);
    const float inv_gamma = 1.f / k.gamma, scale = k.gamma * k.invstd;
    float mdz = 0.f, mdzx = 0.f;                                  // sum dz / n and sum dz xhat / n (training only)
    if (saved) {
        double s1 = 0.0, s2 = 0.0;
        for (int r = 0; r < R; ++r) {
            s1 += all_sums[(size_t)r * 2 * C + c];
            s2 += all_sums[(size_t)r * 2 * C + C + c];
        }
        const double n = saved[2 * C + c];
        mdz = (float)(s1 / n);
        mdzx = (float)(s2 / n);
    }
    const bool need_y = source == kFromInput && op.act != kIdentity;
    const bool need_r = source == kFromOutput && res != nullptr;
    const size_t base = plane * HW, f0 = base + (size_t)chunk * kBlockElems;
    const size_t f1 = base + ((size_t)(chunk + 1) * kBlockElems < (size_t)HW ? (size_t)(chunk + 1) * kBlockElems : HW);
    const size_t g1 = (f1 + V - 1) / V;
    for (size_t gb = f0 / V + threadIdx.x; gb < g1; gb += (size_t)kThreads * U) {
        float vs[U][V], vy[U][V], vd[U][V], vr[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t g = gb + (size_t)u * kThreads;
            if (g >= g1) continue;
            const bool full = vec && g * V >= f0 && g * V + V <= f1;
            load_group(src, g, f0, f1, full, vs[u]);
            load_group(dy, g, f0, f1, full, vd[u]);
            if (need_y) load_group(y, g, f0, f1, full, vy[u]);
            if (need_r) load_group(res, g, f0, f1, full, vr[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t g = gb + (size_t)u * kThreads;
            if (g >= g1) continue;
            const bool full = vec && g * V >= f0 && g * V + V <= f1;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float dz, xhat;
                dz_xhat(source, op, k, inv_gamma, vs[u][e], need_y ? vy[u][e] : 0.f, vd[u][e], need_r ? vr[u][e] : 0.f, dz,
                        xhat);
                vs[u][e] = saved ? scale * (dz - mdz - xhat * mdzx) : scale * dz;
                vd[u][e] = dz;
            }
            store_group(dx, g, f0, f1, full, vs[u]);
            if (dres) store_group(dres, g, f0, f1, full, vd[u]);
        }
    }
}

}  // namespace abn
