// augment_api.hip -- the C ABI of include/ccnet_augment.h (libccnet_augment.so): the descriptor checks and the one launch.
// The launch goes on the caller's stream and nothing waits for the device.
#include "ccnet_augment.h"

#include "augment_kernels.hpp"

#define CCNET_ERROR_PREFIX "ccnet_augment: "
#include "../csrc_common/ccnet_host.hpp"

namespace {

// max(1, round_half_even(n * num / den)) in integers; n <= 2^31 / 1024 is the caller's to keep
long long scaled(long long n, long long num, long long den) {
    const long long p = n * num, q = p / den, r2 = 2 * (p - q * den);
    const long long z = q + ((r2 > den || (r2 == den && (q & 1))) ? 1 : 0);
    return z < 1 ? 1 : z;
}

bool ratio_ok(int num, int den) { return num >= 1 && num <= CCNET_AUGMENT_MAX_RATIO && den >= 1 && den <= CCNET_AUGMENT_MAX_RATIO; }

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ccnet_augment_version(void) { return CCNET_AUGMENT_VERSION; }
__attribute__((visibility("default"))) const char *ccnet_augment_arch(void) { return "gfx950"; }
__attribute__((visibility("default"))) const char *ccnet_augment_last_error_string(void) { return g_err; }

__attribute__((visibility("default"))) int ccnet_augment_scaled_size(int Hs, int Ws, int num, int den, int *hz, int *wz) {
    if (!hz || !wz) return fail(-2, "scaled_size: NULL hz or wz");
    if (!ratio_ok(num, den)) return fail(-1, "scaled_size: scale %d/%d outside 1..%d", num, den, CCNET_AUGMENT_MAX_RATIO);
    if (Hs < 1 || Ws < 1 || Hs > (1 << 20) || Ws > (1 << 20)) return fail(-1, "scaled_size: unsupported frame %d x %d", Hs, Ws);
    const long long H = scaled(Hs, num, den), W = scaled(Ws, num, den);
    if (H > CCNET_AUGMENT_MAX_SIDE || W > CCNET_AUGMENT_MAX_SIDE)
        return fail(-1, "scaled_size: %d x %d at %d/%d is %lld x %lld, above %d", Hs, Ws, num, den, H, W, CCNET_AUGMENT_MAX_SIDE);
    *hz = (int)H;
    *wz = (int)W;
    return 0;
}

__attribute__((visibility("default"))) int ccnet_augment_crop_u8(const uint8_t *frames, size_t frames_bytes, const uint8_t *labels,
                                                                 size_t labels_bytes, const int32_t *desc_host,
                                                                 const int32_t *desc_device, const uint8_t *label_table,
                                                                 float *images, int64_t *out_labels, int B, int crop_h,
                                                                 int crop_w, float mean0, float mean1, float mean2,
                                                                 int ignore_label, int source_rgb, void *stream) {
    if (B < 1 || B > 65535 || crop_h < 1 || crop_w < 1 || crop_h > CCNET_AUGMENT_MAX_SIDE || crop_w > CCNET_AUGMENT_MAX_SIDE ||
        (long long)B * 3 * crop_h * crop_w > 0x7fffffffLL)
        return fail(-1, "crop: unsupported shape B=%d crop %d x %d", B, crop_h, crop_w);
    if (!frames || !labels || !desc_host || !desc_device || !images || !out_labels)
        return fail(-2, "crop: NULL frames, labels, descriptors, images or out_labels");
    for (int b = 0; b < B; ++b) {
        const int32_t *d = desc_host + (size_t)b * CCNET_AUGMENT_DESC_INTS;
        const int Hs = d[CCNET_AUGMENT_HS], Ws = d[CCNET_AUGMENT_WS], pitch = d[CCNET_AUGMENT_PITCH];
        const int num = d[CCNET_AUGMENT_NUM], den = d[CCNET_AUGMENT_DEN], mirror = d[CCNET_AUGMENT_MIRROR];
        if (!ratio_ok(num, den)) return fail(-1, "crop: sample %d: scale %d/%d outside 1..%d", b, num, den, CCNET_AUGMENT_MAX_RATIO);
        int Hz = 0, Wz = 0;
        if (Hs < 1 || Ws < 1 || pitch < Ws || ccnet_augment_scaled_size(Hs, Ws, num, den, &Hz, &Wz) != 0)
            return fail(-1, "crop: sample %d: unsupported frame %d x %d (pitch %d) at scale %d/%d", b, Hs, Ws, pitch, num, den);
        if (d[CCNET_AUGMENT_HZ] != Hz || d[CCNET_AUGMENT_WZ] != Wz)
            return fail(-1, "crop: sample %d: scaled size %d x %d given, %d x %d at scale %d/%d", b, d[CCNET_AUGMENT_HZ],
                        d[CCNET_AUGMENT_WZ], Hz, Wz, num, den);
        const int max_h = (Hz > crop_h ? Hz : crop_h) - crop_h, max_w = (Wz > crop_w ? Wz : crop_w) - crop_w;
        if (d[CCNET_AUGMENT_H_OFF] < 0 || d[CCNET_AUGMENT_H_OFF] > max_h || d[CCNET_AUGMENT_W_OFF] < 0 || d[CCNET_AUGMENT_W_OFF] > max_w)
            return fail(-1, "crop: sample %d: offset (%d, %d) outside [0, %d] x [0, %d]", b, d[CCNET_AUGMENT_H_OFF],
                        d[CCNET_AUGMENT_W_OFF], max_h, max_w);
        if (mirror != 0 && mirror != 1) return fail(-1, "crop: sample %d: mirror flag %d", b, mirror);
        const unsigned long long extent = (unsigned long long)(Hs - 1) * pitch + Ws;     // pixels from the first to past the last
        const long long fo = d[CCNET_AUGMENT_FRAME_OFF], lo = d[CCNET_AUGMENT_LABEL_OFF];
        if (fo < 0 || lo < 0 || fo + 3 * extent > frames_bytes || lo + extent > labels_bytes)
            return fail(-1, "crop: sample %d: frame at %lld or label at %lld (%llu pixels) outside its buffer of %zu / %zu bytes",
                        b, fo, lo, extent, frames_bytes, labels_bytes);
    }
    const dim3 grid((unsigned)((crop_h * crop_w + augment::kThreads - 1) / augment::kThreads), (unsigned)B);
    AUGMENT_LAUNCH(augment::crop_kernel, grid, dim3(augment::kThreads), static_cast<hipStream_t>(stream), frames, labels,
                   desc_device, label_table, images, out_labels, crop_h, crop_w, mean0, mean1, mean2, ignore_label, source_rgb);
    return launched("crop");
}

}  // extern "C"
