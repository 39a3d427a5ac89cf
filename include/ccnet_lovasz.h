/* ccnet_lovasz.h -- C ABI of libccnet_lovasz.so: the Lovász-softmax loss on the device.
 *
 * Semantics of the reference's lovasz_softmax(probas, labels, classes, per_image, ignore) (loss/lovasz_losses.py:18-31,
 * 153-218), with probas (B, C, H, W) fp32 and labels (B, H, W) int64, raw device pointers, contiguous:
 *   1. a pixel is valid when its label != ignore (always when ignore_none is set); pixels are taken in flattened (b, h, w)
 *      order.  Labels outside [0, C) other than ignore stay valid and are background for every class;
 *   2. a segment is one class over one image (per_image) or one class over the whole batch.  For class c:
 *      fg = (label == c), e = |fg - p_c| in fp32.  A class is kept with multiplicity class_weights[c] (NULL: 1 for every
 *      class); present_only additionally drops a class with no fg pixel in the segment;
 *   3. per segment the errors are sorted in descending order -- STABLY: equal errors keep ascending flattened pixel order
 *      (the reference's torch.sort leaves that order unspecified; the loss does not depend on it, the per-pixel gradient
 *      does).  With gts = sum fg, I = gts - cumsum(fg_sorted), U = gts + cumsum(1 - fg_sorted), J = 1 - I / U (prefix counts
 *      exact integers converted to fp32, correctly rounded fp32 division), g[0] = J[0], g[i] = J[i] - J[i-1]:
 *      loss_seg = sum e_sorted * g;
 *   4. loss = the weighted mean of loss_seg over the kept classes; per_image: the mean over images of each image's mean.
 *      An empty class set, or an image without a valid pixel, contributes 0 with zero gradient (the reference returns an
 *      empty tensor there);
 *   5. backward: d loss / d p_c = grad_out * g[rank] * (-sign(fg - p_c)) * weight / n_kept (/ B per image), sign(0) = 0;
 *      0 on pixels that are not valid and on classes that are not kept.
 * g is bit-identical to the reference's for the same sorted fg up to 2^24 pixels per segment; longer segments are rejected.
 *
 * Every launch goes on `stream` (NULL = the default stream); nothing synchronises with the host and the class selection
 * travels in the kernel arguments (no host-to-device copy).  The caller provides the workspace
 * (ccnet_lovasz_workspace_bytes, about 20.5 bytes per pixel and class: double-buffered 32-bit sort keys and payloads, the
 * per-pixel Lovász gradient, per-tile counts); backward reads what forward left in it, so the same workspace goes to both
 * and stays untouched in between.  Reductions are deterministic (fixed-order partials in double, no float atomics).
 * Return codes: 0 ok, -1 bad shape or parameter (2 <= C <= 256, a segment of at most 2^24 pixels), -2 NULL pointer,
 * -3 workspace too small, -4 launch failure (ccnet_lovasz_last_error_string says which).
 */
#ifndef CCNET_LOVASZ_H
#define CCNET_LOVASZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCNET_LOVASZ_VERSION 100

int ccnet_lovasz_version(void);
const char *ccnet_lovasz_arch(void);
const char *ccnet_lovasz_last_error_string(void);

/* bytes of workspace forward + backward need for this shape (0 on a bad shape) */
size_t ccnet_lovasz_workspace_bytes(int B, int C, int H, int W, int per_image);

/* loss[0] <- the Lovász-softmax loss; n_kept[0] <- the kept class count (weights included, summed over images when
   per_image), optional (NULL: not written).  class_weights is a HOST array of C multiplicities (0..255) or NULL. */
int ccnet_lovasz_forward_f32(const float *probas, const int64_t *labels, float *loss, int *n_kept, void *workspace,
                             size_t workspace_bytes, int B, int C, int H, int W, long long ignore, int ignore_none,
                             int per_image, int present_only, const unsigned char *class_weights, void *stream);

/* grad_probas <- grad_out[0] * d loss / d probas; grad_out is a device scalar. */
int ccnet_lovasz_backward_f32(const float *grad_out, float *grad_probas, const void *workspace, size_t workspace_bytes,
                              int B, int C, int H, int W, int per_image, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CCNET_LOVASZ_H */
