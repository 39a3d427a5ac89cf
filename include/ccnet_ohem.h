/* ccnet_ohem.h -- C ABI of libccnet_ohem.so: online hard example mining (OHEM) cross-entropy on the device.
 *
 * Semantics of the reference's OhemCrossEntropy2d(ignore_label, thresh, min_kept, factor) (loss/loss.py:9-93):
 *   1. softmax over C; the label's own probability is zoomed by 1/factor (linear, scipy.ndimage.zoom order 1,
 *      grid_mode=False) and the labels with order 0; output length round(n / factor), source coordinate
 *      o * (n - 1) / (n_out - 1) in double;
 *   2. over the whole batch, with k = min_kept / factor^2 and num_valid the zoomed labels != ignore_label:
 *      threshold = 1 if k >= num_valid, else max(thresh, k-th smallest zoomed target probability) (thresh alone if k == 0);
 *   3. a full-resolution pixel is kept when its label is valid and its fp32 softmax target probability <= threshold;
 *      loss = mean over kept pixels of -log p_target (F.cross_entropy with the other pixels ignored: NaN when none is kept).
 * Labels outside [0, C) other than ignore_label count as ignored.
 *
 * All tensors are raw device pointers, contiguous: logits (B, C, H, W) fp32, labels (B, H, W) int64.  Every launch goes on
 * `stream` (NULL = the default stream); nothing synchronises with the host.  The caller provides the workspace
 * (ccnet_ohem_workspace_bytes); backward reads what forward left in it, so the same workspace must be passed to both and
 * stay untouched in between.  Reduction is deterministic (fixed-order block partials, no float atomics).
 * Return codes: 0 ok, -1 bad shape or parameter, -2 NULL pointer, -3 workspace too small, -4 launch failure
 * (ccnet_ohem_last_error_string says which).
 */
#ifndef CCNET_OHEM_H
#define CCNET_OHEM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCNET_OHEM_VERSION 100

int ccnet_ohem_version(void);
const char *ccnet_ohem_arch(void);
const char *ccnet_ohem_last_error_string(void);

/* bytes of workspace forward + backward need for this shape (0 on a bad shape) */
size_t ccnet_ohem_workspace_bytes(int B, int C, int H, int W, int factor);

/* loss[0] <- the OHEM cross-entropy; threshold[0], kept[0] (full-resolution pixels kept) and num_valid[0] (valid zoomed
   labels) <- the statistics of this call, each optional (NULL: not written). */
int ccnet_ohem_forward_f32(const float *logits, const int64_t *labels, float *loss, float *threshold, int *kept,
                           int *num_valid, void *workspace, size_t workspace_bytes, int B, int C, int H, int W,
                           long long ignore_label, float thresh, int min_kept, int factor, void *stream);

/* grad_logits <- grad_out[0] * (softmax - onehot) / kept on kept pixels, 0 elsewhere; grad_out is a device scalar. */
int ccnet_ohem_backward_f32(const float *grad_out, const float *logits, float *grad_logits, const void *workspace,
                            size_t workspace_bytes, int B, int C, int H, int W, int factor, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CCNET_OHEM_H */
