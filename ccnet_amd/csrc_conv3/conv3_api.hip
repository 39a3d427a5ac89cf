// conv3_api.hip -- extern "C" entry points of libccnet_conv3.so (see include/ccnet_conv3.h).
//
// Built for the device with   hipcc --offload-arch=gfx950 -O3 -shared -fPIC -I. -I../csrc -I../../include
// (__graft_entry__.build()); the headers of ../csrc are read, never changed.  The CPU test-suite compiles this same file with the
// host compiler against tests/emu/ and tests/emu_conv3/ (first on its include path) to execute the kernels in the SIMT emulator;
// that build is test-only.
#include "../../include/ccnet_conv3.h"

#include "conv3_kernels.hpp"

#include <stdio.h>

#include <string>

namespace {

thread_local std::string g_last_error = "";

int fail(int code, const char *what) {
    char buf[256];
    snprintf(buf, sizeof(buf), "ccnet_conv3: %s (code %d)", what, code);
    g_last_error = buf;
    return code;
}

// CONV3_LAUNCH clears the sticky error of earlier, unrelated HIP calls before launching, so what is read here belongs to the
// launch just issued
int launch_status(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[256];
        snprintf(buf, sizeof(buf), "ccnet_conv3: launch of %s failed: %s", what, hipGetErrorString(e));
        g_last_error = buf;
        return (int)e;
    }
    return 0;
}

constexpr double kMaxElems = 1073741824.0;          // 2^30 bf16 elements = 2^31 bytes
constexpr int kWorkgroups = 256;                    // the CU count the slab rule aims at: a constant, not the device's (same bits everywhere)

bool aligned4(const void *p) { return ((uintptr_t)p & 3u) == 0; }

bool image_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && (double)B * H * W < kMaxElems; }

long wgrad_tiles(int N, int C) { return (long)((N + cca::PW_BN - 1) / cca::PW_BN) * ((C + cca::PW_BC - 1) / cca::PW_BC); }

// slabs of the weight gradient: S * 9 * tiles ~ kWorkgroups, S = 1 where the tiles alone exceed it; at least 64 rows per slab
int wgrad_slabs(long R, int N, int C) {
    const long per = conv3::kTaps * wgrad_tiles(N, C), most = (R + 63) / 64;
    long S = per >= kWorkgroups ? 1 : kWorkgroups / per;
    if (S > most) S = most;
    return (int)(S < 1 ? 1 : S);
}

bool wgrad_shape_ok(int B, int H, int W, int N, int C) {
    return image_ok(B, H, W) && N > 0 && C > 0 && N % 8 == 0 && C % 8 == 0 && (double)N * C < kMaxElems / 2;
}

}  // namespace

extern "C" {

int ccnet_conv3_version(void) { return CCNET_CONV3_VERSION; }
const char *ccnet_conv3_arch(void) { return "gfx950"; }
const char *ccnet_conv3_last_error(void) { return g_last_error.c_str(); }

int ccnet_conv3_bf16(const uint16_t *a, const uint16_t *wt, const float *bias, const uint16_t *add, uint16_t *out,
                     int B, int H, int W, int K, int N, int dilation, long lda, long ldadd, long ldo, ccnet_conv3_stream_t stream) {
    if (!a || !wt || !out) return fail(CCNET_CONV3_E_NULLPTR, "conv3_bf16: null tensor");
    if (!image_ok(B, H, W) || N <= 0 || K <= 0 || K % 8 || N % 4)
        return fail(CCNET_CONV3_E_BADSHAPE, "conv3_bf16: B, H, W, N, K > 0, K % 8 == 0, N % 4 == 0");
    if (dilation < 1) return fail(CCNET_CONV3_E_BADSHAPE, "conv3_bf16: dilation >= 1");
    if (lda % 8 || ldo % 4 || lda < K || ldo < N) return fail(CCNET_CONV3_E_BADSHAPE, "conv3_bf16: lda % 8 == 0, ldo % 4 == 0, strides >= extents");
    if (add && (ldadd % 4 || ldadd < N)) return fail(CCNET_CONV3_E_BADSHAPE, "conv3_bf16: ldadd % 4 == 0, ldadd >= N");
    if (!aligned4(a) || !aligned4(wt) || !aligned4(out) || !aligned4(add) || !aligned4(bias))
        return fail(CCNET_CONV3_E_BADSHAPE, "conv3_bf16: pointers are 4-byte aligned");
    const int M = B * H * W;
    if ((double)M * lda >= kMaxElems || (double)N * conv3::kTaps * K >= kMaxElems || (double)M * ldo >= kMaxElems
        || (add && (double)M * ldadd >= kMaxElems))
        return fail(CCNET_CONV3_E_BADSHAPE, "conv3_bf16: a byte offset of the launch reaches 2^31 (cut the batch into several calls)");
    const long tiles = (long)((M + cca::PG_BM - 1) / cca::PG_BM) * ((N + cca::PG_BN - 1) / cca::PG_BN);
    if (tiles >= 2147483647L) return fail(CCNET_CONV3_E_BADSHAPE, "conv3_bf16: too many tiles");
    // (a dilation of max(H, W) or more reaches no pixel but the centre: clamped, so that no displacement overflows)
    const int reach = H > W ? H : W, d = dilation < reach ? dilation : reach;
    const conv3::ConvJob job{(const cca::bf16_t *)a, (const cca::bf16_t *)wt, bias, (const cca::bf16_t *)add, (cca::bf16_t *)out,
                             M, N, K, (int)lda, add ? (int)ldadd : 0, (int)ldo, H, W, d};
    if (K % cca::PG_BK) CONV3_LAUNCH(conv3::conv3_bf16_kernel<true>, dim3((unsigned)tiles), dim3(cca::PG_THREADS), stream, job);
    else                CONV3_LAUNCH(conv3::conv3_bf16_kernel<false>, dim3((unsigned)tiles), dim3(cca::PG_THREADS), stream, job);
    return launch_status("conv3_bf16");
}

int ccnet_conv3_pack(const void *weight, int dtype, uint16_t *fwd, uint16_t *adj, int Cout, int Cin, ccnet_conv3_stream_t stream) {
    if (!weight || !fwd || !adj) return fail(CCNET_CONV3_E_NULLPTR, "pack: null tensor");
    if (dtype != CCNET_CONV3_BF16 && dtype != CCNET_CONV3_F32) return fail(CCNET_CONV3_E_BADFLAGS, "pack: dtype is CCNET_CONV3_BF16 or CCNET_CONV3_F32");
    if (Cout <= 0 || Cin <= 0 || (double)Cout * Cin * conv3::kTaps >= kMaxElems) return fail(CCNET_CONV3_E_BADSHAPE, "pack: channel counts");
    const long items = (long)Cout * Cin * conv3::kTaps;
    const unsigned gx = (unsigned)((items + 255) / 256 < 4096 ? (items + 255) / 256 : 4096);
    if (dtype == CCNET_CONV3_F32)
        CONV3_LAUNCH(conv3::pack_kernel<float>, dim3(gx), dim3(256), stream, weight, (cca::bf16_t *)fwd, (cca::bf16_t *)adj, Cout, Cin);
    else
        CONV3_LAUNCH(conv3::pack_kernel<cca::bf16_t>, dim3(gx), dim3(256), stream, weight, (cca::bf16_t *)fwd, (cca::bf16_t *)adj, Cout, Cin);
    return launch_status("pack");
}

int ccnet_conv3_wgrad_slabs(int B, int H, int W, int N, int C) {
    if (!wgrad_shape_ok(B, H, W, N, C)) return 0;
    return wgrad_slabs((long)B * H * W, N, C);
}

size_t ccnet_conv3_wgrad_workspace_bytes(int B, int H, int W, int N, int C, int slabs) {
    if (!wgrad_shape_ok(B, H, W, N, C) || slabs < 0) return 0;
    const int S = slabs ? slabs : wgrad_slabs((long)B * H * W, N, C);
    return (size_t)S * conv3::kTaps * (size_t)N * (size_t)C * sizeof(float);
}

int ccnet_conv3_wgrad_bf16(const uint16_t *dy, const uint16_t *x, void *workspace, size_t workspace_bytes, int B, int H, int W,
                           int N, int C, int dilation, long ldd, long ldx, int slabs, ccnet_conv3_stream_t stream) {
    if (!dy || !x) return fail(CCNET_CONV3_E_NULLPTR, "wgrad_bf16: null tensor");
    if (!wgrad_shape_ok(B, H, W, N, C)) return fail(CCNET_CONV3_E_BADSHAPE, "wgrad_bf16: B, H, W, N, C > 0, N % 8 == 0, C % 8 == 0");
    if (dilation < 1) return fail(CCNET_CONV3_E_BADSHAPE, "wgrad_bf16: dilation >= 1");
    if (ldd % 8 || ldx % 8 || ldd < N || ldx < C || !aligned4(dy) || !aligned4(x))
        return fail(CCNET_CONV3_E_BADSHAPE, "wgrad_bf16: ldd, ldx % 8 == 0, strides >= extents, 4-byte aligned rows");
    const long R = (long)B * H * W;
    if ((double)R * ldd >= kMaxElems || (double)R * ldx >= kMaxElems)
        return fail(CCNET_CONV3_E_BADSHAPE, "wgrad_bf16: a byte offset of the launch reaches 2^31 (cut the batch into several calls)");
    if (slabs < 0 || slabs > 65536) return fail(CCNET_CONV3_E_BADFLAGS, "wgrad_bf16: 0 <= slabs <= 65536");
    const int S = slabs ? slabs : wgrad_slabs(R, N, C);
    const long groups = (long)S * conv3::kTaps * wgrad_tiles(N, C);
    if (groups >= 2147483647L) return fail(CCNET_CONV3_E_BADSHAPE, "wgrad_bf16: too many workgroups");
    if (!workspace || ((uintptr_t)workspace & 15u) || workspace_bytes < ccnet_conv3_wgrad_workspace_bytes(B, H, W, N, C, S))
        return fail(CCNET_CONV3_E_WORKSPACE, "wgrad_bf16: workspace missing, misaligned or too small (ccnet_conv3_wgrad_workspace_bytes)");
    const long slab = ((R + S - 1) / S + 63) / 64 * 64;
    const int reach = H > W ? H : W, d = dilation < reach ? dilation : reach;
    const conv3::WgradJob job{(const cca::bf16_t *)dy, (const cca::bf16_t *)x, (float *)workspace, (int)R, N, C, (int)ldd, (int)ldx, S,
                              (int)slab, H, W, d};
    CONV3_LAUNCH(conv3::conv3_wgrad_kernel, dim3((unsigned)groups), dim3(cca::PG_THREADS), stream, job);
    return launch_status("wgrad_bf16");
}

int ccnet_conv3_wgrad_finish(const void *workspace, void *dw, int dtype, int N, int C, int slabs, ccnet_conv3_stream_t stream) {
    if (!workspace || !dw) return fail(CCNET_CONV3_E_NULLPTR, "wgrad_finish: null tensor");
    if (dtype != CCNET_CONV3_BF16 && dtype != CCNET_CONV3_F32)
        return fail(CCNET_CONV3_E_BADFLAGS, "wgrad_finish: dtype is CCNET_CONV3_BF16 or CCNET_CONV3_F32");
    if (N <= 0 || C <= 0 || slabs <= 0 || (double)N * C >= kMaxElems / 2) return fail(CCNET_CONV3_E_BADSHAPE, "wgrad_finish: N, C, slabs > 0");
    const long NC = (long)N * C;
    const unsigned gx = (unsigned)((NC + 255) / 256 < 4096 ? (NC + 255) / 256 : 4096);
    if (dtype == CCNET_CONV3_F32)
        CONV3_LAUNCH(conv3::wgrad_finish_kernel<float>, dim3(gx), dim3(256), stream, (const float *)workspace, (float *)dw, NC, slabs);
    else
        CONV3_LAUNCH(conv3::wgrad_finish_kernel<cca::bf16_t>, dim3(gx), dim3(256), stream, (const float *)workspace, (cca::bf16_t *)dw, NC, slabs);
    return launch_status("wgrad_finish");
}

}  // extern "C"
