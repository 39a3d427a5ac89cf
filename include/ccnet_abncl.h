/* ccnet_abncl.h -- C ABI of libccnet_abncl.so: activated batch normalisation (ABN) on a pixel-major (channels_last) tensor.
 *
 * The arithmetic is include/ccnet_abn.h's, function for function; only the layout differs.  Tensors (x, y, dy, dx, the
 * residual and dresidual) are dense (M, C) matrices, row-major with row stride C, M = N * H * W pixels and C channels: what
 * a dense torch.channels_last (N, C, H, W) tensor is in memory.  fp32 or bf16 (desc->dtype), fp32 weight, bias and running
 * statistics, raw device pointers.  Everything ccnet_abn.h states holds here with "per channel over (N, H, W)" read as "per
 * column over the M rows":
 *   statistics  ccnet_abncl_stats writes this rank's (count = M, mean, M2) per channel in fp64; ccnet_abncl_stats_combine
 *               merges R ranks' triples in rank order (Chan), writes saved = (mean, invstd, count) and updates the running
 *               statistics (unbiased running variance, n the global count);
 *   forward     y = act(gamma (x - mean) invstd + beta [+ residual]); saved == NULL: eval mode on the running statistics;
 *               y may alias x (in place);
 *   gamma       CCNET_ABNCL_GAMMA_WEIGHT: gamma = weight; CCNET_ABNCL_GAMMA_ABS_EPS: gamma = |weight| + eps.  weight / bias
 *               NULL: gamma = 1 (+ eps under ABS_EPS), beta = 0;
 *   activation  identity; relu; leaky_relu(p), p >= 0; elu(p), p > 0; d act / dz is taken from y;
 *   backward    dz = dy act'(y); xhat from the input (CCNET_ABNCL_FROM_INPUT: src = x, y for act' unless identity) or
 *               rebuilt from the output (CCNET_ABNCL_FROM_OUTPUT: src = y; leaky p > 0, elu, identity; relu is rejected;
 *               elu's inverse clamps y / p at -1 + 2^-24).  ccnet_abncl_backward_reduce: sums[0:C] = sum dz,
 *               sums[C:2C] = sum dz xhat (fp64), dbias = sum dz, dweight = sum dz xhat (times sign(weight) under ABS_EPS),
 *               all local to this rank.  ccnet_abncl_backward_apply: dx = gamma invstd (dz - sum dz / n - xhat sum dz xhat
 *               / n) with the R ranks' sums added in rank order and n the saved count; eval mode: dx = gamma invstd dz;
 *               dresidual = dz when requested.  dx must not alias dy.
 * local, saved, sums and the rank tables have ccnet_abn.h's shapes and meaning, so one exchange serves both libraries.
 *
 * Every reduction is a fixed-order tree: a workgroup takes a tile of channels (at least 128 bytes of a row where C allows)
 * and a slab of consecutive rows, each thread keeps fp64 sums for its own channels (shifted by the channel's row-0 value for
 * the statistics), the threads of a column are added in index order and the slabs in slab order by a finalize kernel.  The
 * slab count (ccnet_abncl_splits) depends on (M, C, dtype) alone.  No float atomics; results repeat bit for bit, and a
 * 16-byte aligned call gives the bits of a misaligned one.  The workspace (ccnet_abncl_workspace_bytes: 16 bytes per channel
 * and slab) holds the partials between the two kernels of a call.  The tolerance bars and the in-place rounding bounds are
 * ccnet_abn.h's.  A NaN or an infinity in x stays in its own channel.
 *
 * No host synchronisation; every launch on `stream` (NULL = the default stream).
 * Return codes: 0 ok, -1 bad descriptor or argument, -2 NULL pointer, -3 workspace too small, -4 launch failure
 * (ccnet_abncl_last_error_string says which).
 */
#ifndef CCNET_ABNCL_H
#define CCNET_ABNCL_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCNET_ABNCL_VERSION 100

#define CCNET_ABNCL_F32 0
#define CCNET_ABNCL_BF16 1

#define CCNET_ABNCL_IDENTITY 0
#define CCNET_ABNCL_RELU 1
#define CCNET_ABNCL_LEAKY_RELU 2
#define CCNET_ABNCL_ELU 3

#define CCNET_ABNCL_GAMMA_WEIGHT 0
#define CCNET_ABNCL_GAMMA_ABS_EPS 1

#define CCNET_ABNCL_FROM_INPUT 0
#define CCNET_ABNCL_FROM_OUTPUT 1

typedef struct ccnet_abncl_desc {
    int dtype;          /* CCNET_ABNCL_F32 or CCNET_ABNCL_BF16 */
    long long M;        /* rows (pixels): 1 <= M < 2^31, M * C < 2^40 */
    int C;              /* columns (channels): >= 1 */
    int activation;     /* CCNET_ABNCL_IDENTITY ... CCNET_ABNCL_ELU */
    float act_param;    /* leaky_relu slope or elu alpha */
    int gamma_mode;     /* CCNET_ABNCL_GAMMA_WEIGHT or CCNET_ABNCL_GAMMA_ABS_EPS */
    float eps;          /* >= 0; > 0 under ABS_EPS */
} ccnet_abncl_desc;

int ccnet_abncl_version(void);
const char *ccnet_abncl_arch(void);
const char *ccnet_abncl_last_error_string(void);

/* bytes of workspace ccnet_abncl_stats and ccnet_abncl_backward_reduce need (0 on a bad descriptor) */
size_t ccnet_abncl_workspace_bytes(const ccnet_abncl_desc *d);

/* the number of row slabs the reductions cut M into, which fixes their summation order (0 on a bad descriptor) */
int ccnet_abncl_splits(const ccnet_abncl_desc *d);

/* local (3 x C fp64) <- this rank's (count, mean, M2) per channel */
int ccnet_abncl_stats(const ccnet_abncl_desc *d, const void *x, double *local, void *workspace, size_t workspace_bytes,
                      void *stream);

/* saved (3 x C fp64) <- (mean, invstd, count) of the R ranks' triples all (R x 3 x C fp64) merged in rank order; running_mean
   and running_var (fp32, either may be NULL) updated with `momentum` */
int ccnet_abncl_stats_combine(const ccnet_abncl_desc *d, const double *all, int R, float momentum, float *running_mean,
                              float *running_var, double *saved, void *stream);

/* y <- act(gamma (x - mean) invstd + beta [+ residual]); saved NULL: eval mode on the running statistics */
int ccnet_abncl_forward(const ccnet_abncl_desc *d, const void *x, const void *residual, void *y, const double *saved,
                        const float *running_mean, const float *running_var, const float *weight, const float *bias,
                        void *stream);

/* sums (2 x C fp64) <- this rank's (sum dz, sum dz xhat); dweight, dbias (fp32, either may be NULL) <- the local gradients */
int ccnet_abncl_backward_reduce(const ccnet_abncl_desc *d, int source, const void *src, const void *y, const void *dy,
                                const void *residual, const double *saved, const float *running_mean,
                                const float *running_var, const float *weight, const float *bias, double *sums,
                                float *dweight, float *dbias, void *workspace, size_t workspace_bytes, void *stream);

/* dx <- the input gradient from all_sums (R x 2 x C fp64; unused in eval mode); dresidual (may be NULL) <- dz */
int ccnet_abncl_backward_apply(const ccnet_abncl_desc *d, int source, const void *src, const void *y, const void *dy,
                               const void *residual, const double *saved, const float *running_mean,
                               const float *running_var, const float *weight, const float *bias, const double *all_sums,
                               int R, void *dx, void *dresidual, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CCNET_ABNCL_H */
