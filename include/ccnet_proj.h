/* ccnet_proj.h -- C ABI of libccnet_proj.so: the stacked 1x1 projections of the criss-cross attention module on bf16
 * activations (functions.py:29,32,35 and their adjoints) as the library's own MFMA GEMM for gfx950, plus the weight packer and
 * the bias-gradient column sums that go with it.  A library of its own beside libccnet_cca.so (whose symbol set is closed).
 *
 * Every tensor argument is a raw device pointer; every launch goes on the caller's stream; no entry point synchronises, allocates
 * or keeps state.  Entry points return 0 or a negative CCNET_PROJ_E_* code (a positive value is a hipError_t of a launch); argument
 * errors are reported BEFORE any launch, ccnet_proj_last_error() describes the last one of the calling thread.
 */
#ifndef CCNET_PROJ_H
#define CCNET_PROJ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the functions declared here -- and nothing else -- are its dynamic symbols. */
#pragma GCC visibility push(default)

#define CCNET_PROJ_VERSION 100

#define CCNET_PROJ_E_BADSHAPE (-1)  /* extents, strides, alignment, or a byte offset of the launch >= 2^31 */
#define CCNET_PROJ_E_NULLPTR (-2)
#define CCNET_PROJ_E_BADFLAGS (-3)
#define CCNET_PROJ_E_WORKSPACE (-4)

#define CCNET_PROJ_BF16 0           /* parameter element types of ccnet_proj_pack */
#define CCNET_PROJ_F32 1

typedef void *ccnet_proj_stream_t;  /* hipStream_t */

int ccnet_proj_version(void);
const char *ccnet_proj_arch(void);
const char *ccnet_proj_last_error(void);

/* out[m][n] = bf16_rne( sum_k a[m][k] * wt[n][k] + bias[n] + add[m][n] ), fp32 accumulation that STARTS from bias + addend, one
 * rounding to bf16 (round to nearest even, torch's conversion).
 *   a   (M, K) bf16, row stride lda          wt  (N, K) bf16, row stride ldw          (both K-contiguous)
 *   bias (N) fp32 or NULL                    add (M, N) bf16, row stride ldadd, or NULL
 *   out (M, N) bf16, row stride ldo
 * Contract: K % 8 == 0, N % 4 == 0, lda % 8 == 0, ldw % 8 == 0, ldo % 4 == 0, ldadd % 4 == 0 (elements), strides >= extents,
 * pointers 4-byte aligned, and every byte offset of the launch below 2^31 (M * lda, N * ldw, M * ldo, M * ldadd < 2^30 elements):
 * longer inputs are cut into launches over row ranges by the caller. */
int ccnet_proj_gemm_bf16(const uint16_t *a, const uint16_t *wt, const float *bias, const uint16_t *add, uint16_t *out,
                         int M, int N, int K, long lda, long ldw, long ldadd, long ldo, ccnet_proj_stream_t stream);

/* The stacked projection operands of one module application from the six parameter tensors (dtype CCNET_PROJ_BF16 or _F32, all
 * six alike; fp32 values are rounded to nearest even): w (2 Cq + C, C) bf16 = [wq; wk; wv], wt (C, 2 Cq + C) bf16 = its
 * transpose, b (2 Cq + C) fp32 = [bq; bk; bv].  One launch. */
int ccnet_proj_pack(const void *wq, const void *bq, const void *wk, const void *bk, const void *wv, const void *bv, int dtype,
                    uint16_t *w, uint16_t *wt, float *b, int C, int Cq, ccnet_proj_stream_t stream);

/* db[n] = sum_m d[m][n] over the bf16 rows of d (M, N), row stride ldd (N % 4 == 0, ldd % 4 == 0, M * ldd < 2^30), accumulated in
 * double in a fixed order -- partial sums of row slabs, then one finishing workgroup -- and written as fp32: no atomics, the same
 * bits every run.  ``workspace``: ccnet_proj_colsum_workspace_bytes(M, N) bytes, 8-byte aligned, any content. */
size_t ccnet_proj_colsum_workspace_bytes(int M, int N);
int ccnet_proj_colsum_bf16(const uint16_t *d, float *db, int M, int N, long ldd, void *workspace, size_t workspace_bytes,
                           ccnet_proj_stream_t stream);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif
