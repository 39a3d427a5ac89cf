/* ccnet_conv3.h -- C ABI of libccnet_conv3.so: the 3x3, stride-1, dilated convolution (padding = dilation, groups 1) on bf16
 * channels_last activations as an implicit GEMM on the library's own MFMA kernels for gfx950: forward and input gradient (one
 * kernel), weight gradient (slab partials + a finishing launch) and the weight packer.  A library of its own beside
 * libccnet_cca.so and libccnet_proj.so, whose headers it reads and whose code it leaves alone.
 *
 * Every tensor argument is a raw device pointer; every launch goes on the caller's stream; no entry point synchronises, allocates
 * or keeps state.  Entry points return 0 or a negative CCNET_CONV3_E_* code (a positive value is a hipError_t of a launch); argument
 * errors are reported BEFORE any launch, ccnet_conv3_last_error() describes the last one of the calling thread.
 *
 * Pixels are rows: row r = (b * H + h) * W + w of B whole images.  Tap t = 3 (ky + 1) + (kx + 1), ky, kx in {-1, 0, 1};
 * src(r, t) is the pixel (h + ky d, w + kx d) of the SAME image and contributes zero when it lies outside the image.
 */
#ifndef CCNET_CONV3_H
#define CCNET_CONV3_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the functions declared here -- and nothing else -- are its dynamic symbols. */
#pragma GCC visibility push(default)

#define CCNET_CONV3_VERSION 100

#define CCNET_CONV3_E_BADSHAPE (-1)  /* extents, strides, alignment, or a byte offset of the launch >= 2^31 */
#define CCNET_CONV3_E_NULLPTR (-2)
#define CCNET_CONV3_E_BADFLAGS (-3)
#define CCNET_CONV3_E_WORKSPACE (-4)

#define CCNET_CONV3_BF16 0           /* element types of the parameter (pack) and of its gradient (wgrad_finish) */
#define CCNET_CONV3_F32 1

typedef void *ccnet_conv3_stream_t;  /* hipStream_t */

int ccnet_conv3_version(void);
const char *ccnet_conv3_arch(void);
const char *ccnet_conv3_last_error(void);

/* out[r][n] = bf16_rne( sum_t sum_c a[src(r,t)][c] * wt[n][t K + c] + bias[n] + add[r][n] ), fp32 accumulation that STARTS from
 * bias + addend, one rounding to bf16 (round to nearest even).
 *   a   (B H W, K) bf16, row stride lda            wt  (N, 9 K) bf16, contiguous (K-contiguous within a tap)
 *   bias (N) fp32 or NULL                          add (B H W, N) bf16, row stride ldadd, or NULL
 *   out (B H W, N) bf16, row stride ldo
 * Forward: a = x, K = Cin, N = Cout, wt = the forward pack.  Input gradient: a = dy, K = Cout, N = Cin, wt = the adjoint pack.
 * Contract: K % 8 == 0, N % 4 == 0, lda % 8 == 0, ldo % 4 == 0, ldadd % 4 == 0 (elements), strides >= extents, pointers 4-byte
 * aligned, dilation >= 1, and every byte offset of the launch below 2^31 (B H W * lda, N * 9 K, B H W * ldo, B H W * ldadd < 2^30
 * elements): longer inputs are cut at image boundaries by the caller, which is exact. */
int ccnet_conv3_bf16(const uint16_t *a, const uint16_t *wt, const float *bias, const uint16_t *add, uint16_t *out,
                     int B, int H, int W, int K, int N, int dilation, long lda, long ldadd, long ldo, ccnet_conv3_stream_t stream);

/* Both packs of a contiguous (Cout, Cin, 3, 3) parameter (dtype CCNET_CONV3_BF16: copied, or _F32: rounded to nearest even) in
 * one launch:  fwd (Cout, 9 Cin): fwd[n][t Cin + c] = w[n][c][t];   adj (Cin, 9 Cout): adj[c][t Cout + n] = w[n][c][8 - t]. */
int ccnet_conv3_pack(const void *weight, int dtype, uint16_t *fwd, uint16_t *adj, int Cout, int Cin, ccnet_conv3_stream_t stream);

/* The weight gradient.  part[s][t][n][c] = sum over the rows r of slab s of dy[r][n] * x[src(r,t)][c], fp32; the rows are cut
 * into S slabs of ceil(B H W / S) rows rounded up to a multiple of 64 (a slab may be empty: its partials are zeros).  ``slabs``
 * 0: S = ccnet_conv3_wgrad_slabs(...), a function of the shape alone; > 0: that many.  Every element of part (S, 9, N, C) is
 * written.  No atomics: the same bits every run.
 *   dy (B H W, N) bf16, row stride ldd             x (B H W, C) bf16, row stride ldx
 * Contract: N % 8 == 0, C % 8 == 0, ldd % 8 == 0, ldx % 8 == 0, strides >= extents, B H W * stride < 2^30 elements.
 * ``workspace`` = part: ccnet_conv3_wgrad_workspace_bytes(...) bytes, 16-byte aligned, any content. */
int ccnet_conv3_wgrad_slabs(int B, int H, int W, int N, int C);
size_t ccnet_conv3_wgrad_workspace_bytes(int B, int H, int W, int N, int C, int slabs);
int ccnet_conv3_wgrad_bf16(const uint16_t *dy, const uint16_t *x, void *workspace, size_t workspace_bytes, int B, int H, int W,
                           int N, int C, int dilation, long ldd, long ldx, int slabs, ccnet_conv3_stream_t stream);

/* dw[n][c][t] = sum_s part[s][t][n][c], the S partials added in slab order in fp32, written in the parameter's own layout
 * (N = Cout, C = Cin, 3, 3) as bf16 (one rounding to nearest even) or as fp32 (unrounded), by ``dtype``. */
int ccnet_conv3_wgrad_finish(const void *workspace, void *dw, int dtype, int N, int C, int slabs, ccnet_conv3_stream_t stream);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif
