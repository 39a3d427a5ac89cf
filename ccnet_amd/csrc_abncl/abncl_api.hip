// abncl_api.hip -- the C ABI of include/ccnet_abncl.h (libccnet_abncl.so): argument checks, grids, launches.
// Every launch goes on the caller's stream and nothing waits for the device.
#include "ccnet_abncl.h"

#include <math.h>
#include <stdint.h>

#include "abncl_kernels.hpp"

#define CCNET_ERROR_PREFIX "ccnet_abncl: "
#include "../csrc_common/ccnet_host.hpp"

namespace {

struct Grid {
    abncl::Geo geo, ew;              // the reductions' slabs (at most kMaxSlabs) and the elementwise passes' row blocks
    int V;
    unsigned blocks, ew_blocks, chan_blocks;
    size_t ws;
};

// `cap` (or fewer) blocks of consecutive rows: about kTargetBlocks workgroups over `tiles`, at least kMinRows rows each, none empty
void cut_rows(long long M, long long tiles, long long cap, long long &S, long long &chunk) {
    S = (abncl::kTargetBlocks + tiles - 1) / tiles;
    const long long by_size = (M + abncl::kMinRows - 1) / abncl::kMinRows;
    if (S > by_size) S = by_size;
    if (S > cap) S = cap;
    if (S < 1) S = 1;
    chunk = (M + S - 1) / S;
    S = (M + chunk - 1) / chunk;
}

// 0 or the failing code (with g_err set)
int plan(const ccnet_abncl_desc *d, const char *what, Grid &g) {
    if (!d) return fail(-2, "%s: NULL descriptor", what);
    if (d->dtype != CCNET_ABNCL_F32 && d->dtype != CCNET_ABNCL_BF16) return fail(-1, "%s: dtype %d", what, d->dtype);
    if (d->M < 1 || d->C < 1) return fail(-1, "%s: bad shape M=%lld C=%d", what, d->M, d->C);
    if (d->M >= (1ll << 31) || d->M * d->C >= (1ll << 40))
        return fail(-1, "%s: shape M=%lld C=%d too large", what, d->M, d->C);
    if (d->activation < CCNET_ABNCL_IDENTITY || d->activation > CCNET_ABNCL_ELU)
        return fail(-1, "%s: activation %d", what, d->activation);
    if (!isfinite(d->act_param) || (d->activation == CCNET_ABNCL_LEAKY_RELU && d->act_param < 0.f) ||
        (d->activation == CCNET_ABNCL_ELU && !(d->act_param > 0.f)))
        return fail(-1, "%s: activation parameter %g (leaky_relu >= 0, elu > 0)", what, (double)d->act_param);
    if (d->gamma_mode != CCNET_ABNCL_GAMMA_WEIGHT && d->gamma_mode != CCNET_ABNCL_GAMMA_ABS_EPS)
        return fail(-1, "%s: gamma_mode %d", what, d->gamma_mode);
    if (!isfinite(d->eps) || d->eps < 0.f || (d->gamma_mode == CCNET_ABNCL_GAMMA_ABS_EPS && !(d->eps > 0.f)))
        return fail(-1, "%s: eps %g (>= 0; > 0 with gamma |weight| + eps)", what, (double)d->eps);
    g.V = d->dtype == CCNET_ABNCL_F32 ? 4 : 8;
    // the tile: the smallest power of two of 16-byte groups that covers a row, at most 128 bytes
    const long long groups = ((long long)d->C + g.V - 1) / g.V;
    int CG = 1;
    while (CG < groups && CG < abncl::kMaxGroups) CG *= 2;
    const long long TC = (long long)CG * g.V, tiles = (d->C + TC - 1) / TC;
    long long S, chunk, S_ew, chunk_ew;
    cut_rows(d->M, tiles, abncl::kMaxSlabs, S, chunk);
    cut_rows(d->M, tiles, abncl::kTargetBlocks, S_ew, chunk_ew);
    if (tiles * S_ew >= (1ll << 31)) return fail(-1, "%s: shape M=%lld C=%d needs too many workgroups", what, d->M, d->C);
    g.geo.M = d->M;
    g.geo.chunk = chunk;
    g.geo.C = d->C;
    g.geo.S = (int)S;
    g.geo.CG = CG;
    g.ew = g.geo;
    g.ew.chunk = chunk_ew;
    g.ew.S = (int)S_ew;
    g.blocks = (unsigned)(tiles * S);
    g.ew_blocks = (unsigned)(tiles * S_ew);
    g.chan_blocks = (unsigned)((d->C + abncl::kThreads - 1) / abncl::kThreads);
    g.ws = (size_t)d->C * (size_t)S * 2 * sizeof(double);
    return 0;
}

abn::Op op_of(const ccnet_abncl_desc *d) {
    abn::Op op;
    op.act = d->activation;
    op.p = d->act_param;
    op.abs_eps = d->gamma_mode == CCNET_ABNCL_GAMMA_ABS_EPS;
    op.eps = d->eps;
    return op;
}

bool aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_source(const ccnet_abncl_desc *d, int source, const char *what) {
    if (source != CCNET_ABNCL_FROM_INPUT && source != CCNET_ABNCL_FROM_OUTPUT) return fail(-1, "%s: source %d", what, source);
    if (source == CCNET_ABNCL_FROM_OUTPUT &&
        (d->activation == CCNET_ABNCL_RELU || (d->activation == CCNET_ABNCL_LEAKY_RELU && !(d->act_param > 0.f))))
        return fail(-1, "%s: the input cannot be rebuilt from the output of relu or leaky_relu with slope 0", what);
    return 0;
}

template <class T>
void run_stats(const Grid &g, const void *x, double *local, void *ws, int vec, hipStream_t s) {
    const T *xt = static_cast<const T *>(x);
    double *part = static_cast<double *>(ws);
    ABN_LAUNCH(abncl::stats_partial_kernel<T>, dim3(g.blocks), dim3(abncl::kThreads), s, xt, part, g.geo, vec);
    // (N, C, HW) = (M, C, 1): the channel's first element is x[c], the count M
    ABN_LAUNCH(abn::stats_finalize_kernel<T>, dim3(g.chan_blocks), dim3(abncl::kThreads), s, xt, (const double *)part, local,
               (int)g.geo.M, g.geo.C, 1, g.geo.S);
}

template <class T>
void run_forward(const ccnet_abncl_desc *d, const Grid &g, const void *x, const void *res, void *y, const double *saved,
                 const float *rm, const float *rv, const float *w, const float *b, int vec, hipStream_t s) {
    ABN_LAUNCH(abncl::forward_kernel<T>, dim3(g.ew_blocks), dim3(abncl::kThreads), s, static_cast<const T *>(x),
               static_cast<const T *>(res), static_cast<T *>(y), saved, rm, rv, w, b, g.ew, op_of(d), vec);
}

template <class T>
void run_reduce(const ccnet_abncl_desc *d, const Grid &g, int source, const void *src, const void *y, const void *dy,
                const void *res, const double *saved, const float *rm, const float *rv, const float *w, const float *b,
                double *sums, float *dw, float *db, void *ws, int vec, hipStream_t s) {
    double *part = static_cast<double *>(ws);
    ABN_LAUNCH(abncl::backward_partial_kernel<T>, dim3(g.blocks), dim3(abncl::kThreads), s, static_cast<const T *>(src),
               static_cast<const T *>(y), static_cast<const T *>(dy), static_cast<const T *>(res), saved, rm, rv, w, b, part,
               g.geo, op_of(d), source, vec);
    ABN_LAUNCH(abn::backward_finalize_kernel, dim3(g.chan_blocks), dim3(abncl::kThreads), s, (const double *)part, w, sums, dw,
               db, g.geo.C, g.geo.S, d->gamma_mode == CCNET_ABNCL_GAMMA_ABS_EPS ? 1 : 0);
}

template <class T>
void run_apply(const ccnet_abncl_desc *d, const Grid &g, int source, const void *src, const void *y, const void *dy,
               const void *res, const double *saved, const float *rm, const float *rv, const float *w, const float *b,
               const double *all_sums, int R, void *dx, void *dres, int vec, hipStream_t s) {
    ABN_LAUNCH(abncl::backward_apply_kernel<T>, dim3(g.ew_blocks), dim3(abncl::kThreads), s, static_cast<const T *>(src),
               static_cast<const T *>(y), static_cast<const T *>(dy), static_cast<const T *>(res), saved, rm, rv, w, b,
               all_sums, R, static_cast<T *>(dx), static_cast<T *>(dres), g.ew, op_of(d), source, vec);
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ccnet_abncl_version(void) { return CCNET_ABNCL_VERSION; }
__attribute__((visibility("default"))) const char *ccnet_abncl_arch(void) { return "gfx950"; }
__attribute__((visibility("default"))) const char *ccnet_abncl_last_error_string(void) { return g_err; }

__attribute__((visibility("default"))) size_t ccnet_abncl_workspace_bytes(const ccnet_abncl_desc *d) {
    Grid g;
    return plan(d, "workspace_bytes", g) == 0 ? g.ws : 0;
}

__attribute__((visibility("default"))) int ccnet_abncl_splits(const ccnet_abncl_desc *d) {
    Grid g;
    return plan(d, "splits", g) == 0 ? g.geo.S : 0;
}

__attribute__((visibility("default"))) int ccnet_abncl_stats(const ccnet_abncl_desc *d, const void *x, double *local,
                                                             void *workspace, size_t workspace_bytes, void *stream) {
    Grid g;
    if (int e = plan(d, "stats", g)) return e;
    if (!x || !local || !workspace) return fail(-2, "stats: NULL x, local or workspace");
    if (workspace_bytes < g.ws) return fail(-3, "stats: workspace of %zu bytes, %zu needed", workspace_bytes, g.ws);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int vec = d->C % g.V == 0 && aligned(x);
    if (d->dtype == CCNET_ABNCL_F32)
        run_stats<float>(g, x, local, workspace, vec, s);
    else
        run_stats<uint16_t>(g, x, local, workspace, vec, s);
    return launched("stats");
}

__attribute__((visibility("default"))) int ccnet_abncl_stats_combine(const ccnet_abncl_desc *d, const double *all, int R,
                                                                     float momentum, float *running_mean,
                                                                     float *running_var, double *saved, void *stream) {
    Grid g;
    if (int e = plan(d, "stats_combine", g)) return e;
    if (R < 1) return fail(-1, "stats_combine: R = %d ranks", R);
    if (!isfinite(momentum)) return fail(-1, "stats_combine: momentum %g", (double)momentum);
    if (!all || !saved) return fail(-2, "stats_combine: NULL all or saved");
    ABN_LAUNCH(abn::stats_combine_kernel, dim3(g.chan_blocks), dim3(abncl::kThreads), static_cast<hipStream_t>(stream), all, R,
               d->C, d->eps, momentum, running_mean, running_var, saved);
    return launched("stats_combine");
}

__attribute__((visibility("default"))) int ccnet_abncl_forward(const ccnet_abncl_desc *d, const void *x,
                                                               const void *residual, void *y, const double *saved,
                                                               const float *running_mean, const float *running_var,
                                                               const float *weight, const float *bias, void *stream) {
    Grid g;
    if (int e = plan(d, "forward", g)) return e;
    if (!x || !y) return fail(-2, "forward: NULL x or y");
    if (!saved && (!running_mean || !running_var))
        return fail(-2, "forward: eval mode (saved NULL) needs running_mean and running_var");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int vec = d->C % g.V == 0 && aligned(x) && aligned(y) && (!residual || aligned(residual));
    if (d->dtype == CCNET_ABNCL_F32)
        run_forward<float>(d, g, x, residual, y, saved, running_mean, running_var, weight, bias, vec, s);
    else
        run_forward<uint16_t>(d, g, x, residual, y, saved, running_mean, running_var, weight, bias, vec, s);
    return launched("forward");
}

__attribute__((visibility("default"))) int ccnet_abncl_backward_reduce(
    const ccnet_abncl_desc *d, int source, const void *src, const void *y, const void *dy, const void *residual,
    const double *saved, const float *running_mean, const float *running_var, const float *weight, const float *bias,
    double *sums, float *dweight, float *dbias, void *workspace, size_t workspace_bytes, void *stream) {
    Grid g;
    if (int e = plan(d, "backward_reduce", g)) return e;
    if (int e = check_source(d, source, "backward_reduce")) return e;
    const bool need_y = source == CCNET_ABNCL_FROM_INPUT && d->activation != CCNET_ABNCL_IDENTITY;
    if (!src || !dy || !sums || !workspace || (need_y && !y))
        return fail(-2, "backward_reduce: NULL src, dy, sums or workspace (or y, needed for act')");
    if (!saved && (!running_mean || !running_var))
        return fail(-2, "backward_reduce: eval mode (saved NULL) needs running_mean and running_var");
    if (workspace_bytes < g.ws)
        return fail(-3, "backward_reduce: workspace of %zu bytes, %zu needed", workspace_bytes, g.ws);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int vec = d->C % g.V == 0 && aligned(src) && aligned(dy) && (!need_y || aligned(y)) &&
                    (!residual || aligned(residual));
    if (d->dtype == CCNET_ABNCL_F32)
        run_reduce<float>(d, g, source, src, y, dy, residual, saved, running_mean, running_var, weight, bias, sums, dweight,
                          dbias, workspace, vec, s);
    else
        run_reduce<uint16_t>(d, g, source, src, y, dy, residual, saved, running_mean, running_var, weight, bias, sums,
                             dweight, dbias, workspace, vec, s);
    return launched("backward_reduce");
}

__attribute__((visibility("default"))) int ccnet_abncl_backward_apply(
    const ccnet_abncl_desc *d, int source, const void *src, const void *y, const void *dy, const void *residual,
    const double *saved, const float *running_mean, const float *running_var, const float *weight, const float *bias,
    const double *all_sums, int R, void *dx, void *dresidual, void *stream) {
    Grid g;
    if (int e = plan(d, "backward_apply", g)) return e;
    if (int e = check_source(d, source, "backward_apply")) return e;
    const bool need_y = source == CCNET_ABNCL_FROM_INPUT && d->activation != CCNET_ABNCL_IDENTITY;
    if (!src || !dy || !dx || (need_y && !y)) return fail(-2, "backward_apply: NULL src, dy or dx (or y, needed for act')");
    if (saved && (!all_sums || R < 1)) return fail(-2, "backward_apply: training mode needs all_sums of R >= 1 ranks");
    if (!saved && (!running_mean || !running_var))
        return fail(-2, "backward_apply: eval mode (saved NULL) needs running_mean and running_var");
    if (dx == dy || (dresidual && dresidual == dy)) return fail(-1, "backward_apply: dx and dresidual must not alias dy");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int vec = d->C % g.V == 0 && aligned(src) && aligned(dy) && aligned(dx) && (!need_y || aligned(y)) &&
                    (!residual || aligned(residual)) && (!dresidual || aligned(dresidual));
    if (d->dtype == CCNET_ABNCL_F32)
        run_apply<float>(d, g, source, src, y, dy, residual, saved, running_mean, running_var, weight, bias, all_sums, R, dx,
                         dresidual, vec, s);
    else
        run_apply<uint16_t>(d, g, source, src, y, dy, residual, saved, running_mean, running_var, weight, bias, all_sums, R,
                            dx, dresidual, vec, s);
    return launched("backward_apply");
}

}  // extern "C"
