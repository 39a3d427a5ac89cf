// proj_api.hip -- extern "C" entry points of libccnet_proj.so (see include/ccnet_proj.h).
//
// Built for the device with   hipcc --offload-arch=gfx950 -O3 -shared -fPIC -I. -I../csrc   (__graft_entry__.build()); the headers
// of ../csrc are read, never changed.  The CPU test-suite compiles this same file with the host compiler against tests/emu/ and
// tests/emu_proj/ (first on its include path) to execute the kernels in the SIMT emulator; that build is test-only.
#include "../../include/ccnet_proj.h"

#include "proj_kernels.hpp"

#include <stdio.h>

#include <string>

namespace {

thread_local std::string g_last_error = "";

int fail(int code, const char *what) {
    char buf[256];
    snprintf(buf, sizeof(buf), "ccnet_proj: %s (code %d)", what, code);
    g_last_error = buf;
    return code;
}

// PROJ_LAUNCH clears the sticky error of earlier, unrelated HIP calls before launching, so what is read here belongs to the
// launch just issued
int launch_status(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[256];
        snprintf(buf, sizeof(buf), "ccnet_proj: launch of %s failed: %s", what, hipGetErrorString(e));
        g_last_error = buf;
        return (int)e;
    }
    return 0;
}

constexpr double kMaxElems = 1073741824.0;          // 2^30 bf16 elements = 2^31 bytes

bool aligned4(const void *p) { return ((uintptr_t)p & 3u) == 0; }

// slabs of the column sums: a function of the shape alone (the summation order must not depend on the device)
int colsum_slabs(int M, int N) {
    const int gx = (N + proj::CS_COLS - 1) / proj::CS_COLS;
    const int want = (512 + gx - 1) / gx, most = (M + 63) / 64;                // ~two workgroups per CU; at least 64 rows per slab
    return want < most ? want : most;
}

}  // namespace

extern "C" {

int ccnet_proj_version(void) { return CCNET_PROJ_VERSION; }
const char *ccnet_proj_arch(void) { return "gfx950"; }
const char *ccnet_proj_last_error(void) { return g_last_error.c_str(); }

int ccnet_proj_gemm_bf16(const uint16_t *a, const uint16_t *wt, const float *bias, const uint16_t *add, uint16_t *out,
                         int M, int N, int K, long lda, long ldw, long ldadd, long ldo, ccnet_proj_stream_t stream) {
    if (!a || !wt || !out) return fail(CCNET_PROJ_E_NULLPTR, "gemm_bf16: null tensor");
    if (M <= 0 || N <= 0 || K <= 0 || K % 8 || N % 4) return fail(CCNET_PROJ_E_BADSHAPE, "gemm_bf16: M, N, K > 0, K % 8 == 0, N % 4 == 0");
    if (lda % 8 || ldw % 8 || ldo % 4 || lda < K || ldw < K || ldo < N)
        return fail(CCNET_PROJ_E_BADSHAPE, "gemm_bf16: lda, ldw % 8 == 0, ldo % 4 == 0, strides >= extents");
    if (add && (ldadd % 4 || ldadd < N)) return fail(CCNET_PROJ_E_BADSHAPE, "gemm_bf16: ldadd % 4 == 0, ldadd >= N");
    if (!aligned4(a) || !aligned4(wt) || !aligned4(out) || !aligned4(add) || !aligned4(bias))
        return fail(CCNET_PROJ_E_BADSHAPE, "gemm_bf16: pointers are 4-byte aligned");
    if ((double)M * lda >= kMaxElems || (double)N * ldw >= kMaxElems || (double)M * ldo >= kMaxElems || (add && (double)M * ldadd >= kMaxElems))
        return fail(CCNET_PROJ_E_BADSHAPE, "gemm_bf16: a byte offset of the launch reaches 2^31 (cut the rows into several calls)");
    const long tiles = (long)((M + cca::PG_BM - 1) / cca::PG_BM) * ((N + cca::PG_BN - 1) / cca::PG_BN);
    if (tiles >= 2147483647L) return fail(CCNET_PROJ_E_BADSHAPE, "gemm_bf16: too many tiles");
    const proj::GemmJob job{(const cca::bf16_t *)a, (const cca::bf16_t *)wt, bias, (const cca::bf16_t *)add, (cca::bf16_t *)out,
                            M, N, K, (int)lda, (int)ldw, add ? (int)ldadd : 0, (int)ldo};
    if (K % cca::PG_BK) PROJ_LAUNCH(proj::gemm_bf16_kernel<true>, dim3((unsigned)tiles), dim3(cca::PG_THREADS), stream, job);
    else                PROJ_LAUNCH(proj::gemm_bf16_kernel<false>, dim3((unsigned)tiles), dim3(cca::PG_THREADS), stream, job);
    return launch_status("gemm_bf16");
}

int ccnet_proj_pack(const void *wq, const void *bq, const void *wk, const void *bk, const void *wv, const void *bv, int dtype,
                    uint16_t *w, uint16_t *wt, float *b, int C, int Cq, ccnet_proj_stream_t stream) {
    if (!wq || !bq || !wk || !bk || !wv || !bv || !w || !wt || !b) return fail(CCNET_PROJ_E_NULLPTR, "pack: null tensor");
    if (dtype != CCNET_PROJ_BF16 && dtype != CCNET_PROJ_F32) return fail(CCNET_PROJ_E_BADFLAGS, "pack: dtype is CCNET_PROJ_BF16 or CCNET_PROJ_F32");
    if (C <= 0 || Cq <= 0 || (double)(2.0 * Cq + C) * C >= kMaxElems) return fail(CCNET_PROJ_E_BADSHAPE, "pack: channel counts");
    const long items = (long)(2 * Cq + C) * C;
    const unsigned gx = (unsigned)((items + 255) / 256 < 2048 ? (items + 255) / 256 : 2048);
    if (dtype == CCNET_PROJ_F32)
        PROJ_LAUNCH(proj::pack_kernel<float>, dim3(gx), dim3(256), stream, wq, wk, wv, bq, bk, bv, (cca::bf16_t *)w, (cca::bf16_t *)wt, b, C, Cq);
    else
        PROJ_LAUNCH(proj::pack_kernel<cca::bf16_t>, dim3(gx), dim3(256), stream, wq, wk, wv, bq, bk, bv, (cca::bf16_t *)w, (cca::bf16_t *)wt, b, C, Cq);
    return launch_status("pack");
}

size_t ccnet_proj_colsum_workspace_bytes(int M, int N) {
    if (M <= 0 || N <= 0) return 0;
    return (size_t)colsum_slabs(M, N) * (size_t)N * sizeof(double);
}

int ccnet_proj_colsum_bf16(const uint16_t *d, float *db, int M, int N, long ldd, void *workspace, size_t workspace_bytes,
                           ccnet_proj_stream_t stream) {
    if (!d || !db) return fail(CCNET_PROJ_E_NULLPTR, "colsum_bf16: null tensor");
    if (M <= 0 || N <= 0 || N % 4 || ldd % 4 || ldd < N || !aligned4(d))
        return fail(CCNET_PROJ_E_BADSHAPE, "colsum_bf16: M, N > 0, N % 4 == 0, ldd % 4 == 0, ldd >= N, 4-byte aligned rows");
    if ((double)M * ldd >= kMaxElems) return fail(CCNET_PROJ_E_BADSHAPE, "colsum_bf16: a byte offset of the launch reaches 2^31");
    if (!workspace || ((uintptr_t)workspace & 7u) || workspace_bytes < ccnet_proj_colsum_workspace_bytes(M, N))
        return fail(CCNET_PROJ_E_WORKSPACE, "colsum_bf16: workspace missing, misaligned or too small (ccnet_proj_colsum_workspace_bytes)");
    const int S = colsum_slabs(M, N);
    const int slab = (int)(((long)M + S - 1) / S);
    PROJ_LAUNCH(proj::colsum_slab_kernel, dim3((unsigned)((N + proj::CS_COLS - 1) / proj::CS_COLS), (unsigned)S), dim3(proj::CS_THREADS), stream,
                (const cca::bf16_t *)d, (double *)workspace, M, N, (int)ldd, slab);
    if (int e = launch_status("colsum_bf16(slabs)")) return e;
    PROJ_LAUNCH(proj::colsum_finish_kernel, dim3(1), dim3(proj::CF_THREADS), stream, (const double *)workspace, db, N, S);
    return launch_status("colsum_bf16(finish)");
}

}  // extern "C"
