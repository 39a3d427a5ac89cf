/* ccnet_mseval.h -- C ABI of libccnet_mseval.so: multi-scale (plus flip) segmentation evaluation on the device.
 *
 * The reference's entry point is predict_multiscale (evaluate.py:155-175): ndimage.zoom of the image per scale,
 * predict_sliding on the scaled image (and on its mirrored copy), the per-scale maps summed and divided by their number.  As
 * written it cannot add a map of a scale != 1.0 into the full-size array; the missing step, defined here as step 5, is the
 * zoom back by (H / Hs, W / Ws).  Per image n and per scale s, in the caller's order:
 *   1. scaled size: Hs = round(H * s), Ws = round(W * s) with round-half-to-even (what ndimage.zoom produces: 97 x 0.5 -> 48,
 *      97 x 1.5 -> 146, 33 x 0.5 -> 16).  The host computes it; the calls below take Hs, Ws as given.
 *   2. zoom, ndimage.zoom(order=1, prefilter=False): bilinear with the exact end-point ratio.  Output index o of an axis with
 *      n_out positions reads source position o * (n_in - 1) / (n_out - 1), computed in integers:
 *          i0 = o * (n_in - 1) / (n_out - 1),   rem = o * (n_in - 1) % (n_out - 1),
 *          lambda = (float)rem / (float)(n_out - 1),   i1 = min(i0 + 1, n_in - 1);     n_out == 1: i0 = 0, lambda = 0.
 *      One axis: lerp(a, b, lambda) = lambda == 0 ? a : (1 - lambda) * a + lambda * b in fp32; a tap whose weight is exactly 0
 *      contributes nothing and is not read.  Two axes: the lerp along W of each of the two rows, then the lerp of the two
 *      results along H.  (Not PyTorch's fp32 scale * i coordinate: at 2048-4096 columns its error reaches 1e-4 of a pixel.)
 *   3. tiles: the caller's tile grid on the scaled image (whole-image mode: one tile equal to (Hs, Ws)), zero-padded; with
 *      flip the same tiles of the scaled image mirrored along W: column xs of the flipped frame is column Ws - 1 - xs.
 *   4. per-scale score S_s on (Hs, Ws): exactly steps 1-2 of ccnet_eval.h (PyTorch's align_corners=True fp32 arithmetic
 *      inside a tile, fp32 sum in tile order over the count, 0.5 * (plain + flipped) with the flipped pass mirrored back along W).
 *      The zero-weight rule of steps 2 and 5 does NOT hold inside a tile: as in PyTorch, the bilinear sample is the
 *      unconditional sum of its four terms, so a non-finite logit makes S_s non-finite at every position of its tile whose
 *      four neighbours include it, as NaN (0 * inf) where its weight is 0.  Steps 2 and 5 then carry such a position to exactly
 *      the outputs with a non-zero tap weight on it.
 *   5. back to (H, W): R_s = the resample of step 2 from (Hs, Ws) to (H, W), i.e. ndimage.zoom by (H / Hs, W / Ws).  For
 *      Hs == H and Ws == W every weight is exactly 0 or 1 and R_s == S_s bit for bit.
 *   6. combine: score = (sum over s of R_s) / S, summed in fp32 in call order with one fp32 divide at the end; pred = the
 *      first maximum; confusion[label][pred] += 1 when label != ignore_label and 0 <= label < C (ccnet_eval.h steps 3-4).
 *      "First maximum" is np.argmax's: among equal scores the lowest class, and a NaN score counts as the maximum (the first
 *      NaN wins).  The kernel used to skip NaN scores (`s > best` alone); np.argmax is the reference's, so the kernel follows it.
 *      For scores without a NaN nothing changes.  ccnet_eval_sliding_f32 takes its prediction from the same function
 *      (first_maximum, eval_sample.hpp).
 * The divergences of ccnet_eval.h carry over: each image its own tiles, un-flip along W, at least one tile per axis.
 *
 * ccnet_mseval_tiles_f32 is steps 2-3 in one gather kernel: entries [first, first + count) of each image's sequence of T
 * plain tiles followed by T_flip flipped tiles of the scaled image, read straight from the original image (the scaled image
 * is never materialised), every element of tiles_out written (zero where the tile leaves the scaled image).  first / count
 * let the host feed the net in chunks.
 *
 * ccnet_mseval_accumulate_f32 is steps 4-6 for one scale in one kernel: per output pixel, R_s from its <= 4 neighbours in the
 * scaled frame, each evaluated from the covering tiles' low-resolution logits (S_s is never materialised); then
 *     score = score_in ? score_in[..] + R_s : R_s;   if (divide_by > 0) score /= (float)divide_by.
 * score_out is optional and may alias score_in.  pred_out and confusion are computed from that final score: the caller passes
 * them on the last scale only, with divide_by = the number of scales.  labels is required with confusion.
 *
 * Tensors are raw device pointers, contiguous: image fp32 (N, Cin, H, W); tiles_out fp32 (N, count, Cin, tile_H, tile_W);
 * tile_logits fp32 (N, T + T_flip, C, h, w); score_in / score_out fp32 (N, C, H, W); labels int64 (N, H, W); pred_out uint8
 * (N, H, W); confusion int64 (C, C), [label][pred], ACCUMULATED (+=).  tile_y1x1 is a HOST array of 2 * T ints (y1, x1 of each
 * tile of the SCALED image), the same grid for every image and both passes; it travels as a kernel argument.  One launch per
 * call on `stream` (NULL = the default stream); no host synchronisation, no host-to-device copy, no float atomics (the counts
 * go through a per-workgroup LDS histogram of 16-bit counters and integer atomics: deterministic), no scratch.
 * Return codes: 0 ok, -1 bad shape or parameter (C outside [1, 256], T outside [1, 64], T_flip not 0 or T, an origin outside
 * the scaled image, [first, first + count) outside [0, T + T_flip), Hs * Ws or H * W above 2^31 - 1, divide_by < 0), -2 NULL
 * pointer, -4 launch failure (ccnet_mseval_last_error_string says which).
 */
#ifndef CCNET_MSEVAL_H
#define CCNET_MSEVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCNET_MSEVAL_VERSION 100
#define CCNET_MSEVAL_MAX_TILES 64
#define CCNET_MSEVAL_MAX_CLASSES 256

int ccnet_mseval_version(void);
const char *ccnet_mseval_arch(void);
const char *ccnet_mseval_last_error_string(void);

int ccnet_mseval_tiles_f32(const float *image, int N, int Cin, int H, int W, int Hs, int Ws, int T, int T_flip,
                           const int *tile_y1x1, int tile_H, int tile_W, int first, int count, float *tiles_out,
                           void *stream);

int ccnet_mseval_accumulate_f32(const float *tile_logits, int T, int T_flip, const int *tile_y1x1, int N, int C, int h, int w,
                                int tile_H, int tile_W, int Hs, int Ws, int H, int W, const float *score_in, float *score_out,
                                int divide_by, const int64_t *labels, long long ignore_label, uint8_t *pred_out,
                                int64_t *confusion, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CCNET_MSEVAL_H */
