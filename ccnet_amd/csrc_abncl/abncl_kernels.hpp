// abncl_kernels.hpp -- the kernels behind include/ccnet_abncl.h: ABN on a dense (M, C) row-major matrix, M = N * H * W pixels
// (what a dense channels_last tensor is in memory).  The arithmetic is csrc_abn/abn_kernels.hpp's -- Op, Elem<T>, channel(),
// act_forward, act_grad, act_inverse and dz_xhat are included from there and called, not restated -- and so are the three
// per-channel kernels (stats_finalize with HW = 1, stats_combine, backward_finalize), which only see the partials.
//
// One partition serves the reductions and the elementwise passes:
//   group      V consecutive channels of one row, 16 bytes: V = 4 fp32 or 8 bf16.  One vector load or store when C % V == 0 and
//              the call's tensor pointers are 16-byte aligned (every row then starts on a 16-byte boundary), element by element
//              otherwise; a row's last group is short when C % V != 0.  Thread <-> group assignment and every summation order
//              are the same in both forms, so they give the same bits.
//   tile       CG groups side by side, CG the smallest power of two that covers ceil(C / V), at most kMaxGroups = 8: 128 bytes
//              of a row (64 bf16 or 32 fp32 channels), narrower only when C itself is.
//   slab       `chunk` consecutive rows; S slabs cover M.  S and chunk come from (M, C, dtype) alone (plan() of abncl_api.hip):
//              about kTargetBlocks workgroups per launch, slabs of at least kMinRows rows, and for the reductions at most
//              kMaxSlabs of them (the elementwise passes cut the rows the same way without that cap).
//   workgroup  (tile t, slab s) = blockIdx.x / S, blockIdx.x % S.  Its 256 threads form CG column groups x RL = 256 / CG row
//              lanes, thread = rl * CG + cg: the 8 lanes of a row piece are neighbours, so a wave instruction reads 8 rows x
//              128 bytes.  A thread keeps its column group for the whole launch and walks rows m0 + rl, m0 + rl + RL, ...
//              in batches of U rows whose loads are all issued before the first use (and before the first store: with y
//              aliasing x an element is read and written by the same thread only).
// Reductions: a thread accumulates each of its V channels in fp64 as the NCHW kernels do; the RL row lanes of a column are
// then added through LDS in lane-index order and one fp64 pair per channel and slab goes to part[2 (c S + s)], the layout the
// per-channel finalize kernels read.  Nothing is accumulated through memory; every cross-workgroup dependency is a launch
// boundary.
#pragma once
#include <abn_kernels.hpp>

namespace abncl {

using abn::act_forward;
using abn::Chan;
using abn::channel;
using abn::dz_xhat;
using abn::Elem;
using abn::kFromInput;
using abn::kFromOutput;
using abn::kIdentity;
using abn::kPerThread;
using abn::kThreads;
using abn::Op;

constexpr int kMaxGroups = 8;            // column groups of a tile: 8 x 16 bytes = 128 bytes of a row
constexpr int kTargetBlocks = 2048;      // launches aim at about 8 workgroups per CU ...
constexpr long long kMinRows = 256;      // ... whose slabs hold at least this many rows: 32 KB per 128-byte tile and tensor,
                                         // and at full tile width 8 rows (2 to 4 batches) for every row lane
constexpr int kMaxSlabs = 64;            // slabs of a reduction: the finalize kernels add a channel's S pairs one after the
                                         // other, 0.29 us each on an MI355X (340 us at 1159 slabs, measured), so S is kept
                                         // where that costs less than the partial pass (19 us); the elementwise passes,
                                         // which have no such tail, cut the rows by the first two numbers alone

struct Geo {
    long long M, chunk;                  // rows; rows per slab
    int C, S, CG;                        // channels; slabs; column groups per tile (1, 2, 4 or 8)
};

// a thread's place: channels [c0, c0 + nv) (nv <= 0: its group lies past C), rows m0 + rl + i RL < m1
struct Place {
    long long m0, m1;
    int c0, nv, rl, RL, tile, s;
};
template <int V>
__device__ __forceinline__ Place place(const Geo &g) {
    Place p;
    p.tile = blockIdx.x / g.S;
    p.s = blockIdx.x % g.S;
    p.RL = kThreads / g.CG;
    p.rl = threadIdx.x / g.CG;
    p.c0 = (p.tile * g.CG + threadIdx.x % g.CG) * V;
    p.nv = g.C - p.c0 < V ? g.C - p.c0 : V;
    p.m0 = p.s * g.chunk;
    p.m1 = p.m0 + g.chunk < g.M ? p.m0 + g.chunk : g.M;
    return p;
}

// the group that starts at element `at` = row * C + c0, its first nv channels valid
template <class T>
__device__ __forceinline__ void load_cols(const T *p, size_t at, int nv, int vec, float (&o)[Elem<T>::V]) {
    constexpr int V = Elem<T>::V;
    if (vec) {
        Elem<T>::getv(p, at, o);
        return;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = e < nv ? Elem<T>::get(p, at + e) : 0.f;
}
template <class T>
__device__ __forceinline__ void store_cols(T *p, size_t at, int nv, int vec, const float (&v)[Elem<T>::V]) {
    constexpr int V = Elem<T>::V;
    if (vec) {
        Elem<T>::putv(p, at, v);
        return;
    }
#pragma unroll
    for (int e = 0; e < V; ++e)
        if (e < nv) Elem<T>::put(p, at + e, v[e]);
}

// the row lanes of every column of the tile added in lane-index order; one pair per channel to part[2 (c S + s)].
// thread = rl * CG + cg holds columns cg * V + e of a tile CG * V wide: its slot in row rl of the LDS image is threadIdx.x * V + e
template <int V>
__device__ __forceinline__ void column_sums(const double (&s1)[V], const double (&s2)[V], double *part, const Geo &g,
                                            const Place &p) {
    __shared__ double red[2][kThreads * V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        red[0][threadIdx.x * V + e] = s1[e];
        red[1][threadIdx.x * V + e] = s2[e];
    }
    __syncthreads();
    const int TC = g.CG * V, j = threadIdx.x, c = p.tile * TC + j;
    if (j >= TC || c >= g.C) return;
    double a = red[0][j], b = red[1][j];
    for (int rl = 1; rl < p.RL; ++rl) {
        a += red[0][rl * TC + j];
        b += red[1][rl * TC + j];
    }
    part[2 * ((size_t)c * g.S + p.s)] = a;
    part[2 * ((size_t)c * g.S + p.s) + 1] = b;
}

// shifted sums s1 = sum (x - K), s2 = sum (x - K)^2 in fp64, K = the channel's value in row 0 (what stats_finalize adds back)
template <class T>
__global__ __launch_bounds__(kThreads) void stats_partial_kernel(const T *x, double *part, Geo g, int vec) {
    constexpr int V = Elem<T>::V, U = kPerThread / V;
    const Place p = place<V>(g);
    float K[V];
    double s1[V], s2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        K[e] = e < p.nv ? Elem<T>::get(x, (size_t)(p.c0 + e)) : 0.f;
        s1[e] = s2[e] = 0.0;
    }
    if (p.nv > 0) {
        for (long long rb = p.m0 + p.rl; rb < p.m1; rb += (long long)p.RL * U) {
            float v[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long r = rb + (long long)u * p.RL;
                if (r < p.m1) load_cols(x, (size_t)r * g.C + p.c0, p.nv, vec, v[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (rb + (long long)u * p.RL >= p.m1) continue;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const double d = (double)(v[u][e] - K[e]);      // (a short group's missing channels: 0 - 0)
                    s1[e] += d;
                    s2[e] = fma(d, d, s2[e]);
                }
            }
        }
    }
    column_sums<V>(s1, s2, part, g, p);
}

// the constants of a thread's V channels, computed once
template <int V>
struct Cols {
    Chan k[V];
    float inv_gamma[V], scale[V];
};
template <int V>
__device__ __forceinline__ void columns(Cols<V> &q, const Place &p, int C, const double *saved, const float *rm,
                                        const float *rv, const float *w, const float *b, const Op &op) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
        q.k[e] = e < p.nv ? channel(p.c0 + e, C, saved, rm, rv, w, b, op) : Chan{0.f, 1.f, 1.f, 0.f};
        q.inv_gamma[e] = 1.f / q.k[e].gamma;
        q.scale[e] = q.k[e].gamma * q.k[e].invstd;
    }
}

template <class T>
__global__ __launch_bounds__(kThreads) void forward_kernel(const T *x, const T *res, T *y, const double *saved,
                                                           const float *rm, const float *rv, const float *w, const float *b,
                                                           Geo g, Op op, int vec) {
    constexpr int V = Elem<T>::V, U = kPerThread / V;
    const Place p = place<V>(g);
    if (p.nv <= 0) return;
    Cols<V> q;
    columns<V>(q, p, g.C, saved, rm, rv, w, b, op);
    for (long long rb = p.m0 + p.rl; rb < p.m1; rb += (long long)p.RL * U) {
        float v[U][V], r[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long row = rb + (long long)u * p.RL;
            if (row >= p.m1) continue;
            load_cols(x, (size_t)row * g.C + p.c0, p.nv, vec, v[u]);
            if (res) load_cols(res, (size_t)row * g.C + p.c0, p.nv, vec, r[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long row = rb + (long long)u * p.RL;
            if (row >= p.m1) continue;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float z = (v[u][e] - q.k[e].mean) * q.scale[e] + q.k[e].beta;
                if (res) z += r[u][e];
                v[u][e] = act_forward(z, op.act, op.p);
            }
            store_cols(y, (size_t)row * g.C + p.c0, p.nv, vec, v[u]);
        }
    }
}

// dz = dy act'(y), xhat from x or from y; fp64 partials of sum dz and sum dz xhat
template <class T>
__global__ __launch_bounds__(kThreads) void backward_partial_kernel(const T *src, const T *y, const T *dy, const T *res,
                                                                    const double *saved, const float *rm, const float *rv,
                                                                    const float *w, const float *b, double *part, Geo g,
                                                                    Op op, int source, int vec) {
    constexpr int V = Elem<T>::V, U = kPerThread / V;
    const Place p = place<V>(g);
    const bool need_y = source == kFromInput && op.act != kIdentity;
    const bool need_r = source == kFromOutput && res != nullptr;
    double s1[V], s2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s1[e] = s2[e] = 0.0;
    if (p.nv > 0) {
        Cols<V> q;
        columns<V>(q, p, g.C, saved, rm, rv, w, b, op);
        for (long long rb = p.m0 + p.rl; rb < p.m1; rb += (long long)p.RL * U) {
            float vs[U][V], vy[U][V], vd[U][V], vr[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long row = rb + (long long)u * p.RL;
                if (row >= p.m1) continue;
                const size_t at = (size_t)row * g.C + p.c0;
                load_cols(src, at, p.nv, vec, vs[u]);
                load_cols(dy, at, p.nv, vec, vd[u]);
                if (need_y) load_cols(y, at, p.nv, vec, vy[u]);
                if (need_r) load_cols(res, at, p.nv, vec, vr[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (rb + (long long)u * p.RL >= p.m1) continue;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    if (e >= p.nv) continue;
                    float dz, xhat;
                    dz_xhat(source, op, q.k[e], q.inv_gamma[e], vs[u][e], need_y ? vy[u][e] : 0.f, vd[u][e],
                            need_r ? vr[u][e] : 0.f, dz, xhat);
                    s1[e] += (double)dz;
                    s2[e] = fma((double)dz, (double)xhat, s2[e]);
                }
            }
        }
    }
    column_sums<V>(s1, s2, part, g, p);
}

// dx = gamma invstd (dz - sum dz / n - xhat sum dz xhat / n) (eval: gamma invstd dz); dresidual = dz
template <class T>
__global__ __launch_bounds__(kThreads) void backward_apply_kernel(const T *src, const T *y, const T *dy, const T *res,
                                                                  const double *saved, const float *rm, const float *rv,
                                                                  const float *w, const float *b, const double *all_sums,
                                                                  int R, T *dx, T *dres, Geo g, Op op, int source, int vec) {
    constexpr int V = Elem<T>::V, U = kPerThread / V;
    const Place p = place<V>(g);
    if (p.nv <= 0) return;
    Cols<V> q;
    columns<V>(q, p, g.C, saved, rm, rv, w, b, op);
    float mdz[V], mdzx[V];                                        // sum dz / n and sum dz xhat / n (training only)
#pragma unroll
    for (int e = 0; e < V; ++e) {
        mdz[e] = mdzx[e] = 0.f;
        if (saved && e < p.nv) {
            const int c = p.c0 + e;
            double s1 = 0.0, s2 = 0.0;
            for (int r = 0; r < R; ++r) {
                s1 += all_sums[(size_t)r * 2 * g.C + c];
                s2 += all_sums[(size_t)r * 2 * g.C + g.C + c];
            }
            const double n = saved[2 * g.C + c];
            mdz[e] = (float)(s1 / n);
            mdzx[e] = (float)(s2 / n);
        }
    }
    const bool need_y = source == kFromInput && op.act != kIdentity;
    const bool need_r = source == kFromOutput && res != nullptr;
    for (long long rb = p.m0 + p.rl; rb < p.m1; rb += (long long)p.RL * U) {
        float vs[U][V], vy[U][V], vd[U][V], vr[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long row = rb + (long long)u * p.RL;
            if (row >= p.m1) continue;
            const size_t at = (size_t)row * g.C + p.c0;
            load_cols(src, at, p.nv, vec, vs[u]);
            load_cols(dy, at, p.nv, vec, vd[u]);
            if (need_y) load_cols(y, at, p.nv, vec, vy[u]);
            if (need_r) load_cols(res, at, p.nv, vec, vr[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long row = rb + (long long)u * p.RL;
            if (row >= p.m1) continue;
            const size_t at = (size_t)row * g.C + p.c0;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float dz, xhat;
                dz_xhat(source, op, q.k[e], q.inv_gamma[e], vs[u][e], need_y ? vy[u][e] : 0.f, vd[u][e],
                        need_r ? vr[u][e] : 0.f, dz, xhat);
                vs[u][e] = saved ? q.scale[e] * (dz - mdz[e] - xhat * mdzx[e]) : q.scale[e] * dz;
                vd[u][e] = dz;
            }
            store_cols(dx, at, p.nv, vec, vs[u]);
            if (dres) store_cols(dres, at, p.nv, vec, vd[u]);
        }
    }
}

}  // namespace abncl
