/* ccnet_abn.h -- C ABI of libccnet_abn.so: activated batch normalisation (ABN) on the device, fused and optionally in place.
 *
 * Semantics, for x (N, C, H, W) NCHW-contiguous in fp32 or bf16 (desc->dtype; y, dy, dx and the residual share it), fp32
 * weight, bias and running statistics, raw device pointers:
 *   statistics  mean and biased variance per channel over (N, H, W).  ccnet_abn_stats writes this rank's (count, mean, M2)
 *               in fp64; ccnet_abn_stats_combine merges R ranks' triples IN RANK ORDER with Chan's formula (R = 1 without a
 *               process group), writes saved = (mean, invstd = 1 / sqrt(var + eps), count) in fp64 and updates the running
 *               statistics as F.batch_norm does: rm <- (1 - momentum) rm + momentum mean, rv <- (1 - momentum) rv +
 *               momentum var n / (n - 1), n the global count.  Training on one value per channel is the caller's to reject;
 *   forward     y = act(gamma (x - mean) invstd + beta [+ residual]); eval mode (saved == NULL) takes mean and
 *               invstd = 1 / sqrt(running_var + eps) from the running statistics.  y may alias x (in place);
 *   gamma       CCNET_ABN_GAMMA_WEIGHT: gamma = weight (the stock arithmetic); CCNET_ABN_GAMMA_ABS_EPS: gamma = |weight| + eps,
 *               this library's rule for in-place mode, where the affine step must be invertible.  weight / bias NULL:
 *               gamma = 1 (+ eps under ABS_EPS), beta = 0;
 *   activation  identity; relu; leaky_relu(p), p >= 0; elu(p), p > 0.  d act / dz is taken from y (y > 0: 1; else relu 0,
 *               leaky p, elu y + p);
 *   backward    dz = dy act'(y) and xhat rebuilt per element from either source:
 *               CCNET_ABN_FROM_INPUT:  xhat = (x - mean) invstd from the saved input (src = x, y for act' unless identity);
 *               CCNET_ABN_FROM_OUTPUT: xhat = (act^-1(y) - beta [- residual]) / gamma from the output (src = y, in-place
 *               mode: leaky p > 0, elu, identity; relu has no inverse and is rejected).  elu's inverse clamps y / p at
 *               -1 + 2^-24.
 *               ccnet_abn_backward_reduce: this rank's sums[0:C] = sum dz, sums[C:2C] = sum dz xhat (fp64); dbias = sum dz,
 *               dweight = sum dz xhat (times sign(weight), sign(0) = 0, under ABS_EPS) -- local, as torch's SyncBatchNorm.
 *               ccnet_abn_backward_apply: with the R ranks' sums added in rank order and n = saved count,
 *               dx = gamma invstd (dz - sum dz / n - xhat sum dz xhat / n); eval mode (saved == NULL): dx = gamma invstd dz;
 *               dresidual = dz when requested.  dx must not alias dy.
 * Every reduction is a fixed-order tree of per-workgroup fp64 partials (shifted sums for the statistics, no E[x^2] - E[x]^2
 * in fp32) merged by a finalize kernel: no float atomics, results are bitwise repeatable.  The workspace
 * (ccnet_abn_workspace_bytes: 16 bytes per channel and split) holds the partials between the two kernels of a call; it may
 * be reused by the next call.  Tolerance bar against a float64 oracle of the same arithmetic: fp32 1e-5 relative to the
 * output's scale for y and the statistics, 1e-4 for dweight, dbias and dx (dx against the scale of
 * gamma invstd dz); bf16 tensors: y within 2^-7 and the gradients within 2^-6 of their scale (bf16 rounding of the
 * stored tensors).  For CCNET_ABN_FROM_OUTPUT "the same arithmetic" is the rebuild itself: the oracle starts, as the
 * kernels do, from the y that was stored (rounded to fp32 or bf16) and computes act^-1, xhat, act' and the two sums from it
 * in float64; against that oracle dx and dresidual meet the bar above and dweight, dbias and the sums meet 1e-4 in both
 * dtypes.  Against the EXACT gradients (those of the unrounded forward pass) in-place mode also carries the rounding of the
 * stored y amplified by the inverse activation: not at all for leaky_relu (y / p keeps y's relative rounding), for elu by
 * about e^-z = 1 / (1 + y / p), which grows until y / p reaches the clamp at z = log(2^-24) = -16.6; every z below it is
 * rebuilt as -16.6.  With elu in fp32 the exact dx is met to 1e-4 while z stays above about -16 and is off by 1e-2 of its
 * scale beyond; in bf16 (y + p has 8 bits) by 3e-3 at weight 1 and by a few 1e-2 from weight 4.  dweight and dbias are
 * sums of dz, which elu' = y + p damps where the inverse amplifies, and stay within the bar (DESIGN.md section 14 has the
 * figures).  A NaN or an infinity in x makes its own channel's variance, invstd and running variance NaN and its mean and
 * running mean NaN (or the infinity), as in any batch norm, and leaves every other channel's bits alone.
 *
 * No host synchronisation; every launch on `stream` (NULL = the default stream).
 * Return codes: 0 ok, -1 bad descriptor or argument, -2 NULL pointer, -3 workspace too small, -4 launch failure
 * (ccnet_abn_last_error_string says which).
 */
#ifndef CCNET_ABN_H
#define CCNET_ABN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCNET_ABN_VERSION 100

#define CCNET_ABN_F32 0
#define CCNET_ABN_BF16 1

#define CCNET_ABN_IDENTITY 0
#define CCNET_ABN_RELU 1
#define CCNET_ABN_LEAKY_RELU 2
#define CCNET_ABN_ELU 3

#define CCNET_ABN_GAMMA_WEIGHT 0
#define CCNET_ABN_GAMMA_ABS_EPS 1

#define CCNET_ABN_FROM_INPUT 0
#define CCNET_ABN_FROM_OUTPUT 1

typedef struct ccnet_abn_desc {
    int dtype;          /* CCNET_ABN_F32 or CCNET_ABN_BF16 */
    int N, C, H, W;     /* N * C * H * W < 2^40, H * W < 2^31 */
    int activation;     /* CCNET_ABN_IDENTITY ... CCNET_ABN_ELU */
    float act_param;    /* leaky_relu slope or elu alpha */
    int gamma_mode;     /* CCNET_ABN_GAMMA_WEIGHT or CCNET_ABN_GAMMA_ABS_EPS */
    float eps;          /* >= 0; > 0 under ABS_EPS */
} ccnet_abn_desc;

int ccnet_abn_version(void);
const char *ccnet_abn_arch(void);
const char *ccnet_abn_last_error_string(void);

/* bytes of workspace ccnet_abn_stats and ccnet_abn_backward_reduce need (0 on a bad descriptor) */
size_t ccnet_abn_workspace_bytes(const ccnet_abn_desc *d);

/* local (3 x C fp64) <- this rank's (count, mean, M2) per channel */
int ccnet_abn_stats(const ccnet_abn_desc *d, const void *x, double *local, void *workspace, size_t workspace_bytes,
                    void *stream);

/* saved (3 x C fp64) <- (mean, invstd, count) of the R ranks' triples all (R x 3 x C fp64) merged in rank order; running_mean
   and running_var (fp32, either may be NULL) updated with `momentum` */
int ccnet_abn_stats_combine(const ccnet_abn_desc *d, const double *all, int R, float momentum, float *running_mean,
                            float *running_var, double *saved, void *stream);

/* y <- act(gamma (x - mean) invstd + beta [+ residual]); saved NULL: eval mode on the running statistics */
int ccnet_abn_forward(const ccnet_abn_desc *d, const void *x, const void *residual, void *y, const double *saved,
                      const float *running_mean, const float *running_var, const float *weight, const float *bias,
                      void *stream);

/* sums (2 x C fp64) <- this rank's (sum dz, sum dz xhat); dweight, dbias (fp32, either may be NULL) <- the local gradients */
int ccnet_abn_backward_reduce(const ccnet_abn_desc *d, int source, const void *src, const void *y, const void *dy,
                              const void *residual, const double *saved, const float *running_mean,
                              const float *running_var, const float *weight, const float *bias, double *sums,
                              float *dweight, float *dbias, void *workspace, size_t workspace_bytes, void *stream);

/* dx <- the input gradient from all_sums (R x 2 x C fp64; unused in eval mode); dresidual (may be NULL) <- dz */
int ccnet_abn_backward_apply(const ccnet_abn_desc *d, int source, const void *src, const void *y, const void *dy,
                             const void *residual, const double *saved, const float *running_mean,
                             const float *running_var, const float *weight, const float *bias, const double *all_sums,
                             int R, void *dx, void *dresidual, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CCNET_ABN_H */
