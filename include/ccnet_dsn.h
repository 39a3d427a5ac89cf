/* ccnet_dsn.h -- C ABI of libccnet_dsn.so: the deep-supervision cross-entropy (CriterionDSN, loss/criterion.py:11-35) on
 * low-resolution logits that are up-sampled inside the kernels.
 *
 * Semantics, per head k of `heads` (1 or 2):
 *   up_k = F.interpolate(logits_k, size=(H, W), mode="bilinear", align_corners=True)   -- never materialised
 *   CE_k = F.cross_entropy(up_k, target, ignore_index=ignore_index)                    -- mean over the valid pixels
 *   loss = weight0 * CE_0 (+ weight1 * CE_1)
 * The interpolation is PyTorch's, in fp32 and in its order, along each axis (n_in -> n_out, output index o):
 *   scale = n_out > 1 ? (float)(n_in - 1) / (n_out - 1) : 0;  src = scale * o;  i0 = (int)src;  i1 = i0 + (i0 < n_in - 1);
 *   l1 = src - i0;  l0 = 1 - l1;   value = lh0 * (lw0 * v00 + lw1 * v01) + lh1 * (lw0 * v10 + lw1 * v11).
 * A label other than ignore_index outside [0, C) never indexes anything: the pixel counts as ignored and is counted in
 * counts[1].  With no valid pixel the loss is NaN (0 / 0, as F.cross_entropy) and the gradient is zero everywhere.
 *
 * All tensors are raw device pointers, contiguous: logits (B, C, h, w) fp32, target (B, H, W) int64.  Supported shapes:
 * B >= 1, 1 <= C <= 256, 1 <= h <= H <= 2^20, 1 <= w <= W <= 2^20, B * H * W and B * C * h * w below 2^31, B <= 32767.
 * Every launch goes on `stream` (NULL = the default stream); nothing synchronises with the host and nothing is allocated.
 * The caller provides the workspace (ccnet_dsn_workspace_bytes, at most 16 * B * H * W + 65536 bytes: a log-sum-exp per
 * pixel and head, a two-byte label per pixel and the block partials; nothing of size B * C * H * W exists anywhere).
 * Backward reads what forward left in the workspace, so the same workspace is passed to both and stays untouched in
 * between.  Reductions run in a fixed order and the backward is a gather: no atomics, results bit-identical run to run.
 * Return codes: 0 ok, -1 bad shape or parameter, -2 NULL pointer, -3 workspace too small, -4 launch failure
 * (ccnet_dsn_last_error_string says which).
 */
#ifndef CCNET_DSN_H
#define CCNET_DSN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCNET_DSN_VERSION 100

int ccnet_dsn_version(void);
const char *ccnet_dsn_arch(void);
const char *ccnet_dsn_last_error_string(void);

/* bytes of workspace forward + backward need for this shape (0: unsupported shape) */
size_t ccnet_dsn_workspace_bytes(int B, int C, int h, int w, int H, int W, int heads);

/* loss[0] <- weight0 * CE_0 + weight1 * CE_1; head_loss[0..1] <- CE_0, CE_1 (0 for an absent head); counts[0] <- valid
   pixels, counts[1] <- labels outside [0, C) that are not ignore_index.  head_loss and counts are optional (NULL: not
   written); logits1 is NULL when heads == 1. */
int ccnet_dsn_forward_f32(const float *logits0, const float *logits1, const int64_t *target, float weight0, float weight1,
                          float *loss, float *head_loss, int *counts, void *workspace, size_t workspace_bytes, int B, int C,
                          int h, int w, int H, int W, int heads, long long ignore_index, void *stream);

/* grad_k <- d(grad_out[0] * loss) / d logits_k, every element written; grad_out is a device scalar; logits1 and grad1 are
   NULL when heads == 1. */
int ccnet_dsn_backward_f32(const float *grad_out, const float *logits0, const float *logits1, float *grad0, float *grad1,
                           float weight0, float weight1, const void *workspace, size_t workspace_bytes, int B, int C, int h,
                           int w, int H, int W, int heads, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CCNET_DSN_H */
