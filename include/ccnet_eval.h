/* ccnet_eval.h -- C ABI of libccnet_eval.so: sliding-window segmentation evaluation on the device.
 *
 * One call turns the network's 1/8-resolution tile outputs of a batch of images into the full-resolution score map, the
 * argmax prediction and the confusion counts, with the semantics of the reference's predict_sliding / predict_whole and
 * get_confusion_matrix (evaluate.py:102-143, 145-153, 177-195).  Per pixel (y, x) of image n:
 *   1. for each pass (plain, then flipped when T_flip = T), every tile t whose in-image part covers the pixel contributes the
 *      bilinear, align_corners=True sample of its (h, w) logits up-sampled to (tile_H, tile_W), taken at the pixel's
 *      tile-local position (PyTorch's upsample_bilinear2d arithmetic in fp32: scale = (float)(h - 1) / (tile_H - 1),
 *      source index = scale * i, index0 = (int)source, lambda1 = source - index0, index1 = index0 + (index0 < h - 1));
 *      a tile covers [y1, min(y1 + tile_H, H)) x [x1, min(x1 + tile_W, W)) (a zero-padded tile whose prediction is
 *      cropped, pad_image, evaluate.py:95-100); the samples are summed in fp32 in tile order and divided by their count;
 *      the flipped pass works in the flipped frame: original column x is its column W - 1 - x;
 *   2. with a flipped pass the score is 0.5 * (plain + flipped);
 *   3. pred = the first maximum over the C scores, as np.argmax: among equal scores the lowest class, and a NaN score counts
 *      as the maximum (the first NaN wins).  NaN scores are reachable from a +inf logit: the bilinear sample of step 1 is
 *      PyTorch's unconditional sum of its four terms, so the logit makes the score +inf at the positions of its tile with a
 *      non-zero weight on it and NaN (0 * inf) at those of its four-neighbour footprint with weight 0.  The rule is one
 *      function (first_maximum, eval_sample.hpp) shared with ccnet_mseval_accumulate_f32;
 *   4. confusion[label][pred] += 1 when label != ignore_label and 0 <= label < C.
 * Whole-image evaluation (predict_whole) is the same call with T = 1, origin (0, 0) and tile = image.
 *
 * The call checks that every tile origin lies inside the image, not that the tiles cover it.  A pixel that no tile covers in
 * one of the passes has a count of 0 there and gets 0 / 0: its score is NaN for every class (the other pass's half does not
 * change that), pred = 0 by the rule of step 3, and it is counted at confusion[label][0].  Nothing outside the outputs is
 * read or written for it.  The emulator build and the device agree on this.
 *
 * Deliberate divergences from the reference: every image of a batch gets its own tiles (the reference adds tile 0's
 * prediction to every image of the batch); the flipped pass is mirrored back along W, the axis that was flipped (the
 * reference un-flips along H); the caller's tile grid always has at least one tile per axis (the reference's formula yields
 * none for images far smaller than the tile).
 *
 * Tensors are raw device pointers, contiguous: tile_logits fp32 (N, T + T_flip, C, h, w), the T tiles of image n first, then
 * the T_flip tiles of its horizontally flipped copy; labels int64 (N, H, W); probs_out fp32 (N, C, H, W); pred_out uint8
 * (N, H, W); confusion int64 (C, C), indexed [label][pred] and ACCUMULATED (+=) across calls.  tile_y1x1 is a HOST array of
 * 2 * T ints (y1, x1 of each tile, in the reference's order: rows, then columns), the same grid for every image and for
 * both passes; it travels as a kernel argument.  Every output is optional (NULL: not written); labels is required when
 * confusion is given.  One launch on `stream` (NULL = the default stream); nothing synchronises with the host, nothing is
 * copied host-to-device.  The counts are integer (per-workgroup LDS histogram, integer atomics): deterministic.
 * Return codes: 0 ok, -1 bad shape or parameter (C outside [1, 256], T outside [1, 64], T_flip not 0 or T, an origin outside
 * the image), -2 NULL pointer, -4 launch failure (ccnet_eval_last_error_string says which).
 */
#ifndef CCNET_EVAL_H
#define CCNET_EVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCNET_EVAL_VERSION 100
#define CCNET_EVAL_MAX_TILES 64
#define CCNET_EVAL_MAX_CLASSES 256

int ccnet_eval_version(void);
const char *ccnet_eval_arch(void);
const char *ccnet_eval_last_error_string(void);

int ccnet_eval_sliding_f32(const float *tile_logits, int T, int T_flip, const int *tile_y1x1, int N, int C, int h, int w,
                           int tile_H, int tile_W, int H, int W, const int64_t *labels, long long ignore_label,
                           float *probs_out, uint8_t *pred_out, int64_t *confusion, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CCNET_EVAL_H */
