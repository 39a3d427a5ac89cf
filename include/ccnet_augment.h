/* ccnet_augment.h -- C ABI of libccnet_augment.so: the training input pipeline of dataset/datasets.py (CSDataSet, VOCDataSet:
 * random scale, mean subtraction, bottom/right pad, crop, mirror, label remap) as one gather over packed uint8 frames.
 *
 * Per sample b the caller gives a descriptor of CCNET_AUGMENT_DESC_INTS int32 (layout below): where the frame and its label
 * lie in the packed buffers, the source size Hs x Ws and row pitch, the scale as a rational num/den, the scaled size Hz x Wz,
 * the crop offsets and the mirror flag.  Per call: crop_h x crop_w, three means (in output channel order), ignore_label, an
 * optional 256-entry uint8 label table and the source channel order.  The output is what the reference hands its training
 * loop: images float32 (B, 3, crop_h, crop_w) in BGR order, labels int64 (B, crop_h, crop_w).
 *
 * The arithmetic, all of it in integers (every result is the same in any evaluation order):
 *   scaled size   Hz = max(1, round_half_even(Hs * num / den)), Wz likewise            (cv2.resize(fx, fy)'s cvRound)
 *   output (y,x)  xs = mirror ? crop_w - 1 - x : x;  Y = h_off + y;  X = w_off + xs
 *                 Y >= Hz or X >= Wz: image 0.0f in all three channels, label ignore_label   (the pad comes after the mean
 *                 subtraction in the reference, so the pad value is zero and not -mean)
 *   image         INTER_LINEAR with half-pixel centres, sx = (X + 1/2) * den / num - 1/2, exactly:
 *                   t = (2X + 1) * den - num;  D = 2 * num;  i0 = floor(t / D);  r = t - i0 * D
 *                   t < 0: i0 = 0, r = 0;   i0 >= Ws - 1: i0 = Ws - 1, r = 0;   i1 = min(i0 + 1, Ws - 1)
 *                 rows by the same rule (ry, j0, j1 from Y and Hs).  With p.. the four uint8 taps of one channel:
 *                   n = (p00 * (D - rx) + p01 * rx) * (D - ry) + (p10 * (D - rx) + p11 * rx) * ry
 *                   q = (n + D * D / 2) / (D * D)     (integer division: rounds half up, as a uint8 resize result)
 *                   out = (float)q - mean[c]
 *   label         INTER_NEAREST: sy = min(floor(Y * den / num), Hs - 1), sx likewise; v = label[sy][sx];
 *                 out = (int64)(table ? table[v] : v)
 * Limits, checked before anything is launched: 1 <= num, den <= 1024; 1 <= Hs, Ws <= pitch; Hz, Wz <= 65535 and equal to the
 * formula above; 1 <= crop_h, crop_w <= 65535; 0 <= h_off <= max(Hz, crop_h) - crop_h and likewise w_off; 1 <= B <= 65535;
 * B * 3 * crop_h * crop_w < 2^31; every frame and label inside its buffer.  With them n + D * D / 2 < 2^32 and every
 * intermediate fits 32 bits.
 *
 * frames, labels, label_table, desc_device, images and out_labels are raw device pointers; desc_host is the same table in
 * host memory, which the entry point checks (nothing is read back from the device).  Frames are HWC uint8 with a row pitch
 * of `pitch` pixels (3 * pitch bytes), labels HW uint8 with a row pitch of `pitch` bytes.  No source byte outside
 * [frame_off, frame_off + ((Hs - 1) * pitch + Ws) * 3) and [label_off, label_off + (Hs - 1) * pitch + Ws) is read.  The one
 * launch goes on `stream` (NULL = the default stream); nothing synchronises with the host and nothing is allocated, so the
 * call can be captured into a graph.  Every output element is written.
 * Return codes: 0 ok, -1 bad shape or parameter, -2 NULL pointer, -4 launch failure (ccnet_augment_last_error_string says
 * which).
 */
#ifndef CCNET_AUGMENT_H
#define CCNET_AUGMENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCNET_AUGMENT_VERSION 100

/* one sample's descriptor: int32[CCNET_AUGMENT_DESC_INTS] */
#define CCNET_AUGMENT_DESC_INTS 16
#define CCNET_AUGMENT_FRAME_OFF 0  /* byte offset of the frame's first pixel in `frames` */
#define CCNET_AUGMENT_LABEL_OFF 1  /* byte offset of the label's first pixel in `labels` */
#define CCNET_AUGMENT_HS 2
#define CCNET_AUGMENT_WS 3
#define CCNET_AUGMENT_PITCH 4      /* row pitch of frame and label, in pixels */
#define CCNET_AUGMENT_NUM 5
#define CCNET_AUGMENT_DEN 6
#define CCNET_AUGMENT_HZ 7
#define CCNET_AUGMENT_WZ 8
#define CCNET_AUGMENT_H_OFF 9
#define CCNET_AUGMENT_W_OFF 10
#define CCNET_AUGMENT_MIRROR 11    /* 0 or 1; entries 12..15 are reserved and ignored */

#define CCNET_AUGMENT_MAX_RATIO 1024
#define CCNET_AUGMENT_MAX_SIDE 65535

int ccnet_augment_version(void);
const char *ccnet_augment_arch(void);
const char *ccnet_augment_last_error_string(void);

/* hz[0], wz[0] <- the scaled size of an Hs x Ws frame at num/den; -1 outside the limits above */
int ccnet_augment_scaled_size(int Hs, int Ws, int num, int den, int *hz, int *wz);

/* images (B, 3, crop_h, crop_w) and out_labels (B, crop_h, crop_w) <- the augmented batch.  source_rgb != 0: the frames'
   bytes are R, G, B (PIL); 0: B, G, R (cv2.imread).  label_table may be NULL (identity). */
int ccnet_augment_crop_u8(const uint8_t *frames, size_t frames_bytes, const uint8_t *labels, size_t labels_bytes,
                          const int32_t *desc_host, const int32_t *desc_device, const uint8_t *label_table, float *images,
                          int64_t *out_labels, int B, int crop_h, int crop_w, float mean0, float mean1, float mean2,
                          int ignore_label, int source_rgb, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CCNET_AUGMENT_H */
