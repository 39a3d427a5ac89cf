/* ccnet_ohemdsn.h -- C ABI of libccnet_ohemdsn.so: the OHEM + deep-supervision criterion (CriterionOhemDSN,
 * loss/criterion.py:37-56) on low-resolution logits that are up-sampled inside the kernels.
 *
 * Semantics, with up_k = F.interpolate(logits_k, size=(H, W), mode="bilinear", align_corners=True), never materialised
 * (the interpolation is PyTorch's fp32 arithmetic in its order, as stated in ccnet_dsn.h):
 *   CE_0 = OhemCrossEntropy2d(ignore_index, thresh, min_kept, factor)(up_0, target)   -- loss/loss.py:9-93, as ccnet_ohem.h
 *   CE_1 = F.cross_entropy(up_1, target, ignore_index=ignore_index)                   -- mean over the valid pixels
 *   loss = CE_0 (+ 0.4 * CE_1 when heads == 2)
 * The OHEM threshold is found on scipy's zoom (order 1 of the probabilities, order 0 of the labels, by 1 / factor) of the
 * full-resolution softmax of up_0; every tap of that zoom is interpolated from four low-resolution logits per class on the
 * spot.  A pixel is kept when its label is valid and its own target-class probability is <= threshold; the probability of
 * a tap and of a pixel come from one device function.  A label other than ignore_index outside [0, C) never indexes
 * anything: the pixel counts as ignored and is counted in counts[3].  With nothing kept CE_0 is NaN (0 / 0, as
 * F.cross_entropy) and the gradient of head 0 is zero everywhere; likewise CE_1 and head 1 with no valid pixel.
 *
 * All tensors are raw device pointers, contiguous: logits (B, C, h, w) fp32, target (B, H, W) int64.  Supported: the shapes
 * of ccnet_dsn.h (B >= 1, 1 <= C <= 256, 1 <= h <= H <= 2^20, 1 <= w <= W <= 2^20, B * H * W and B * C * h * w below 2^31,
 * B <= 32767, heads 1 or 2), min_kept >= 0, factor >= 1, thresh not NaN.  Anything else returns a code and launches nothing.
 * Every launch goes on `stream` (NULL = the default stream); nothing synchronises with the host and nothing is allocated.
 * The caller provides the workspace (ccnet_ohemdsn_workspace_bytes, at most
 * 16 * B * H * W + 4 * B * round(H / factor) * round(W / factor) + 65536 bytes: the zoomed keys, a log-sum-exp per pixel
 * and head, a two-byte label per pixel that carries the kept flag, the block partials; nothing of size B * C * H * W exists
 * anywhere).  It starts with the uint32 keys, the fp32 log-sum-exps (one B * H * W plane per head) and the int16 labels
 * (label | 0x100 when head 0 kept the pixel, -1 when the label is not valid), each rounded up to 256 bytes; the rest is
 * private.  Backward reads what forward left in the workspace, so the same workspace is passed to both and stays
 * untouched in between.  Reductions run in a fixed order and the backward is a gather: no float atomics, results
 * bit-identical run to run.
 * Return codes: 0 ok, -1 bad shape or parameter, -2 NULL pointer, -3 workspace too small, -4 launch failure
 * (ccnet_ohemdsn_last_error says which).
 */
#ifndef CCNET_OHEMDSN_H
#define CCNET_OHEMDSN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCNET_OHEMDSN_VERSION 100

int ccnet_ohemdsn_version(void);
const char *ccnet_ohemdsn_arch(void);
const char *ccnet_ohemdsn_last_error(void);

/* bytes of workspace forward + backward need for this shape (0: unsupported shape or factor) */
size_t ccnet_ohemdsn_workspace_bytes(int B, int C, int h, int w, int H, int W, int heads, int factor);

/* loss[0] <- CE_0 + 0.4 * CE_1 (CE_0 with one head); head_loss[0..1] <- CE_0, CE_1 (0 for an absent head); threshold[0] <-
   the OHEM threshold; counts[0..3] <- kept pixels, valid full-resolution pixels, valid zoomed pixels, labels outside [0, C)
   that are not ignore_index.  head_loss, threshold and counts are optional (NULL: not written); logits1 is NULL when
   heads == 1. */
int ccnet_ohemdsn_forward_f32(const float *logits0, const float *logits1, const int64_t *target, long long ignore_index,
                              float thresh, int min_kept, int factor, float *loss, float *head_loss, float *threshold,
                              int *counts, void *workspace, size_t workspace_bytes, int B, int C, int h, int w, int H, int W,
                              int heads, void *stream);

/* grad_k <- d(grad_out[0] * loss) / d logits_k, every element written; grad_out is a device scalar; logits1 and grad1 are
   NULL when heads == 1; factor is the forward's. */
int ccnet_ohemdsn_backward_f32(const float *grad_out, const float *logits0, const float *logits1, float *grad0, float *grad1,
                               const void *workspace, size_t workspace_bytes, int B, int C, int h, int w, int H, int W,
                               int heads, int factor, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CCNET_OHEMDSN_H */
