/* ccnet_celovasz.h -- C ABI of libccnet_celovasz.so: the cross-entropy + Lovász-softmax criterion (CriterionOhemDSN2,
 * loss/criterion.py:59-78) on low-resolution logits that are up-sampled and soft-maxed inside the kernels.
 *
 * Semantics, with up = F.interpolate(logits, size=(H, W), mode="bilinear", align_corners=True), never materialised (the
 * interpolation is PyTorch's fp32 arithmetic in its order, as stated in ccnet_dsn.h), and p = softmax(up) over the classes,
 * never materialised either (p_c = exp(up_c - logsumexp(up)), one device function for the forward and the backward):
 *   CE   = F.cross_entropy(up, target, ignore_index=ignore_index)   -- the mean over the valid pixels; with none valid it is
 *          0 / 0 = NaN, as in ccnet_dsn.h
 *   LS   = lovasz_softmax(p, target, classes, per_image, ignore=ignore_index)   -- rules 2 to 5 of ccnet_lovasz.h unchanged:
 *          the stable tie order, g from exact integer counts and correctly rounded fp32 division, no valid pixel gives 0
 *          with zero gradient; classes travel as present_only and class_weights, as there
 *   loss = CE + LS
 * A pixel is valid when its label lies in [0, C) and is not ignore_index.  A label outside [0, C) other than ignore_index
 * counts as ignored by BOTH terms and is counted in counts[1], as in ccnet_dsn.h and ccnet_ohemdsn.h.  That diverges from rule
 * 1 of ccnet_lovasz.h, which keeps such a pixel valid as background of every class; the reference's cross-entropy raises on
 * it.  With no valid pixel the loss is NaN (CE) and the gradient is zero everywhere, never NaN.
 *
 * Gradient, written once per element by a gather (no atomics):
 *   d loss / d logits[b, c, i, j] = sum over the full-resolution pixels whose footprint holds (i, j) of
 *                                   weight * [ a * (p_c - 1[t = c]) + p_c * (G_c - s) ]
 * with a = grad_out / valid, G_c = d LS / d p_c of rule 5 of ccnet_lovasz.h (0 on classes that are not kept) and
 * s = sum_k p_k * G_k, which the forward leaves in the workspace per pixel (without grad_out; the backward scales).
 *
 * All tensors are raw device pointers, contiguous: logits (B, C, h, w) fp32, target (B, H, W) int64.  Supported: the
 * intersection of ccnet_dsn.h and ccnet_lovasz.h: 1 <= B <= 32767, 2 <= C <= 256, 1 <= h <= H <= 2^20, 1 <= w <= W <= 2^20,
 * a segment (H * W per image, B * H * W otherwise) of at most 2^24 pixels, at most 65535 segments, B * C * h * w below 2^31.
 * Anything else returns a code and launches nothing.  Every launch goes on `stream` (NULL = the default stream); nothing
 * synchronises with the host, nothing is allocated and the class selection travels in the kernel arguments.
 * The caller provides the workspace (ccnet_celovasz_workspace_bytes: at most
 * ccnet_lovasz_workspace_bytes(B, C, H, W, per_image) + 12 * B * H * W + 65536 bytes).  It starts with one fp32 log-sum-exp
 * per pixel and one int16 label per pixel (-1 when the label is not valid), each rounded up to 256 bytes; the rest (s per
 * pixel, the block partials, the scalars, then the Lovász workspace of ccnet_lovasz.h) is private.  Nothing else of size
 * B * C * H * W exists anywhere.  Backward reads what forward left in the workspace and leaves it intact, so the same
 * workspace is passed to both and two backwards from one forward give the same bits.  Reductions run in a fixed order in
 * double; results are bit-identical run to run.
 * Return codes, as ccnet_ohemdsn.h: 0 ok, -1 bad shape or parameter, -2 NULL pointer, -3 workspace too small, -4 launch
 * failure (ccnet_celovasz_last_error says which).
 */
#ifndef CCNET_CELOVASZ_H
#define CCNET_CELOVASZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCNET_CELOVASZ_VERSION 100

int ccnet_celovasz_version(void);
const char *ccnet_celovasz_arch(void);
const char *ccnet_celovasz_last_error(void);

/* bytes of workspace forward + backward need for this shape (0: unsupported shape) */
size_t ccnet_celovasz_workspace_bytes(int B, int C, int h, int w, int H, int W, int per_image);

/* loss[0] <- CE + LS; head_loss[0..1] <- CE, LS; counts[0..2] <- valid pixels, labels outside [0, C) that are not
   ignore_index, the Lovász kept class count (weights included, summed over images when per_image).  head_loss and counts are
   optional (NULL: not written).  class_weights is a HOST array of C multiplicities (0..255) or NULL (1 for every class). */
int ccnet_celovasz_forward_f32(const float *logits, const int64_t *target, long long ignore_index, int per_image,
                               int present_only, const unsigned char *class_weights, float *loss, float *head_loss,
                               int *counts, void *workspace, size_t workspace_bytes, int B, int C, int h, int w, int H, int W,
                               void *stream);

/* grad <- d(grad_out[0] * loss) / d logits, every element written; grad_out is a device scalar. */
int ccnet_celovasz_backward_f32(const float *grad_out, const float *logits, float *grad, const void *workspace,
                                size_t workspace_bytes, int B, int C, int h, int w, int H, int W, int per_image, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CCNET_CELOVASZ_H */
