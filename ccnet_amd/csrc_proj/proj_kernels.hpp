// proj_kernels.hpp -- the kernels of libccnet_proj.so: the module's stacked 1x1 projections on bf16 activations.
//
//     out[m][n] = bf16_rne( sum_k A[m][k] * Wt[n][k] + bias[n] + add[m][n] )      A   (M, K) bf16, row stride lda
//                                                                                 Wt  (N, K) bf16, row stride ldw
//                                                                                 add (M, N) bf16, row stride ldadd, or null
//                                                                                 out (M, N) bf16, row stride ldo
//
// gemm_bf16_kernel is csrc/cca_gemm.hpp's proj_gemm_kernel with ONE bf16 product per term (the operands are bf16 as they come:
// no three-plane rows, K = C) and a bf16 result.  Geometry as there (the constants are that header's): workgroup = 256 x 128
// outputs, 8 wavefronts of 64 x 64 (4 x 4 MFMA tiles, v_mfma_f32_16x16x32_bf16), k steps of 64, both operands K-contiguous =
// T16 row tiles (1 KiB LDS-DMA pieces of 8 rows x 64 k, fragments = one ds_read_b128 per lane), three LDS stages of 48 KiB, the
// register ping-pong over two half steps with the stage barrier between them, XCD-contiguous tile ids with the tiles that share
// a tile of the streamed operand adjacent.  The MFMA operands are SWAPPED (D^T = Wt . A^T): a lane ends with four consecutive n
// of one m.  The accumulators START from bias + addend (fp32); the result is rounded once (v_cvt_pk_bf16_f32, round to nearest
// even) and leaves as 8-byte stores straight from the accumulators: the 16 lanes of a group write 16 rows x 8 bytes, the four
// groups of a wavefront four neighbouring 8-byte columns, i.e. every row of a wavefront's 64 x 64 tile goes out as four 32-byte
// pieces.  (A lane exchange that would build 16-byte stores was not measured; the epilogue is 1/nk of the kernel.)
//
// The loop is proj_gemm_kernel's, waits included (cca_platform.hpp, lds_wait_keep: the reads are outside the compiler's
// bookkeeping, so every path from a read to another mention of its registers passes a wait that names them): the second half's
// fragments are waited for with lgkmcnt(0) BEFORE the branch on "is there a next stage", the last k step requests nothing, and a
// wait after the loop names the first half's registers -- the epilogue may touch any register.  tests/test_isa_hazards.py
// checks the instruction stream for it.
//
// One launch form serves the forward (A = x, K = C, N = 2 Cq + C, bias) and the adjoint with respect to the input (A = dqkv,
// K = 2 Cq + C, N = C, Wt = the transposed stacked weight, add = the residual gradient).  At (16,512,129,129) both are bound by
// HBM: 613 MB moved for 174 GFLOP.
#pragma once
#include "cca_gemm.hpp"

#include <proj_platform.hpp>

namespace proj {

using cca::bf16_t;
using cca::f32x4;
using cca::FBuf;
using cca::kOobOffset;
using cca::kWave;
using cca::PG_APIECES;
using cca::PG_BK;
using cca::PG_BM;
using cca::PG_BN;
using cca::PG_NBUF;
using cca::PG_NPA;
using cca::PG_NPB;
using cca::PG_NPW;
using cca::PG_STAGE;
using cca::PG_THREADS;
using cca::PG_WAVES;
using cca::T16_PIECE;
using cca::u32x4;

struct GemmJob {
    const bf16_t *A, *Wt;
    const float *bias;            // (N) or null
    const bf16_t *add;            // (M, ldadd) or null
    bf16_t *out;
    int M, N, K, lda, ldw, ldadd, ldo;
};

template <bool KTAIL>
__global__ __launch_bounds__(PG_THREADS, 1) void gemm_bf16_kernel(const GemmJob job) {
    __shared__ __attribute__((aligned(16))) float lds[PG_NBUF * PG_STAGE];
    CCA_LDS_REGISTER(lds);
    const int M = job.M, N = job.N, K = job.K, lda = job.lda, ldw = job.ldw, ldo = job.ldo, ldadd = job.ldadd;
    const int ntm = (M + PG_BM - 1) / PG_BM, ntn = (N + PG_BN - 1) / PG_BN;
    const int tl = cca::xcd_logical_id((int)blockIdx.x, (int)gridDim.x);
    // the axis with FEWER tiles runs fastest: the workgroups that share a tile of the other (streamed) operand are neighbours
    const int m0 = (ntn <= ntm ? tl / ntn : tl % ntm) * PG_BM, n0 = (ntn <= ntm ? tl % ntn : tl / ntm) * PG_BN;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = cca::uniform(tid >> 6);
    const int ln = lane & 15, lg = lane >> 4;
    const int wm = wv >> 1, wn = wv & 1;                                       // this wavefront: rows wm * 64 .., columns wn * 64 ..
    const float *bias = job.bias;
    const FBuf Ab = cca::make_fbuf(reinterpret_cast<const float *>(job.A), ((size_t)(M - 1) * lda + K) * 2);
    const FBuf Wb = cca::make_fbuf(reinterpret_cast<const float *>(job.Wt), ((size_t)(N - 1) * ldw + K) * 2);
    const FBuf Ob = cca::make_fbuf(reinterpret_cast<const float *>(job.out), ((size_t)(M - 1) * ldo + N) * 2);
    const FBuf Cb = job.add ? cca::make_fbuf(reinterpret_cast<const float *>(job.add), ((size_t)(M - 1) * ldadd + N) * 2) : Ob;
    const int nk = (K + PG_BK - 1) / PG_BK;

    // fill: wavefront wv moves A pieces wv, wv + 8, .. and Wt pieces wv, wv + 8; lane = (row lane >> 3 of the piece, LDS chunk
    // slot lane & 7), which holds the row's 16-byte k chunk slot ^ row (t16_byte<false>)
    int offa[PG_NPA], offb[PG_NPB];
    {
        const int pr = lane >> 3, q = (lane & 7) ^ pr;
#pragma unroll
        for (int p = 0; p < PG_NPA; ++p) {
            const int r = m0 + 8 * (wv + PG_WAVES * p) + pr;
            offa[p] = ((r < M ? r : M - 1) * lda + 8 * q) * 2;                 // (rows clamped: tail rows are computed, never stored)
        }
#pragma unroll
        for (int p = 0; p < PG_NPB; ++p) {
            const int r = n0 + 8 * (wv + PG_WAVES * p) + pr;
            offb[p] = ((r < N ? r : N - 1) * ldw + 8 * q) * 2;
        }
    }
    const int kq = 8 * ((lane & 7) ^ (lane >> 3));                             // first k of this lane's chunk within a stage
    auto piece = [&](int it, int slot, int i) {                                // fill instruction i of PG_NPW (A pieces first)
        float *as = lds + slot * PG_STAGE + wv * T16_PIECE;
        // (KTAIL, a K that is no multiple of 64: chunks past the end of a row are fetched out of range = zeros)
        const bool dead = KTAIL && it * PG_BK + kq >= K;
        const int koff = it * PG_BK * 2;
        if (i < PG_NPA) cca::fbuf_load_to_lds_x4_uncounted(Ab, as + PG_WAVES * i * T16_PIECE, dead ? kOobOffset : offa[i] + koff);
        else            cca::fbuf_load_to_lds_x4_uncounted(Wb, as + (PG_APIECES + PG_WAVES * (i - PG_NPA)) * T16_PIECE,
                                                           dead ? kOobOffset : offb[i - PG_NPA] + koff);
    };
    auto issue = [&](int it, int slot) {
#pragma unroll
        for (int i = 0; i < PG_NPW; ++i) piece(it, slot, i);
    };
    // fragments of one half step kk (32 k): 8 consecutive k of one row = one 16-byte read; chunk 4 kk + lg of a row lies 64 kk bytes
    // from chunk lg, XORed (t16_byte<false>), the next 16 rows 2 KiB further
    const int fra = cca::t16_byte<false>(wm * 64 + ln, 8 * lg);
    const int frb = cca::t16_byte<false>(wn * 64 + ln, 8 * lg) + PG_APIECES * T16_PIECE * 4;
    auto read = [&](u32x4 (&bf)[4], u32x4 (&af)[4], int slot, int kk) {
        const char *st = reinterpret_cast<const char *>(lds + slot * PG_STAGE);
        const char *pb = st + (frb ^ (64 * kk)), *pa = st + (fra ^ (64 * kk));
        bf[0] = cca::lds_read_x4_uncounted<0>(pb);     bf[1] = cca::lds_read_x4_uncounted<2048>(pb);
        bf[2] = cca::lds_read_x4_uncounted<4096>(pb);  bf[3] = cca::lds_read_x4_uncounted<6144>(pb);
        af[0] = cca::lds_read_x4_uncounted<0>(pa);     af[1] = cca::lds_read_x4_uncounted<2048>(pa);
        af[2] = cca::lds_read_x4_uncounted<4096>(pa);  af[3] = cca::lds_read_x4_uncounted<6144>(pa);
    };

    // D^T[n][m]: lane (ln, lg) of tile (t, j) holds columns n0 + wn * 64 + 16 j + 4 lg .. + 3 of row m0 + wm * 64 + 16 t + ln
    // (N % 4 == 0: the four columns are inside the matrix together or not at all).  The accumulators start from the bias; the
    // addend's 8-byte loads are in flight next to the first three fills and are added before the loop.
    f32x4 acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + 16 * j + 4 * lg;
        f32x4 b4;
#pragma unroll
        for (int q = 0; q < 4; ++q) b4[q] = (bias && n < N) ? bias[n + q] : 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t][j] = b4;
    }
    u32x2v addv[4][4];
    if (job.add) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int m = m0 + wm * 64 + 16 * t + ln;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = n0 + wn * 64 + 16 * j + 4 * lg;
                addv[t][j] = fbuf_load_x2(Cb, (m < M && n < N) ? (m * ldadd + n) * 2 : kOobOffset, 0);
            }
        }
    }

    issue(0, 0);
    if (nk > 1) issue(1, 1);
    if (nk > 2) issue(2, 2);
    if (nk > 2)       cca::barrier_dma_keep<2 * PG_NPW>();                    // stage 0 landed
    else if (nk > 1)  cca::barrier_dma_keep<PG_NPW>();
    else              cca::barrier_dma_keep<0>();
    if (job.add) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t lo = addv[t][j][0], hi = addv[t][j][1];
                acc[t][j] += f32x4{__builtin_bit_cast(float, lo << 16), __builtin_bit_cast(float, lo & 0xffff0000u),
                                   __builtin_bit_cast(float, hi << 16), __builtin_bit_cast(float, hi & 0xffff0000u)};
            }
    }
    u32x4 b0[4], a0[4], b1[4], a1[4];
    read(b0, a0, 0, 0);
    int slot = 0, it = 0;
    do {                                            // (nk >= 1: K > 0 is an argument check; no path skips the loop with reads in flight)
        const int next = slot == PG_NBUF - 1 ? 0 : slot + 1;
        const bool more = it + 1 < nk;
        read(b1, a1, slot, 1);
        cca::lds_wait_keep<8>(b0, a0);             // the first half's fragments are here, the second half's on their way
        cca::sched_fence();                         // (the order is the pipeline: hipcc would otherwise regroup reads and MFMAs)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[t][j] = cca::mfma_bf16_16x16x32(b0[j], a0[t], acc[t][j]);
        cca::sched_fence();
        const bool fill = it + 3 < nk;
        // the second half's fragments are here: a wait for ALL reads, on every path and before the branch (the barrier below waits
        // for lgkmcnt(0) anyway; the last step needs exactly it)
        cca::lds_wait_keep<0>(b1, a1);
        if (more) {
            // stage it + 1 landed and every wavefront holds stage `it` in registers: its slot takes stage it + 3 at once; the
            // fill of stage it + 2 (this wavefront's newest vector-memory operations) stays in flight
            if (it + 2 < nk) cca::barrier_dma_keep<PG_NPW>();
            else             cca::barrier_dma_keep<0>();
            read(b0, a0, next, 0);                  // (the last step requests nothing: there is no next stage)
        }
        cca::sched_fence();
        // second half; the fill instructions of stage it + 3 ride in the shadow of its first MFMAs
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[t][j] = cca::mfma_bf16_16x16x32(b1[j], a1[t], acc[t][j]);
                if (4 * t + j < PG_NPW) {
                    if (fill) piece(it + 3, slot, 4 * t + j);
                    cca::sched_fence();
                }
            }
        cca::sched_fence();
        slot = next;
    } while (++it < nk);
    cca::lds_wait_keep<0>(b0, a0);                  // nothing is outstanding after the loop: the epilogue may touch any register
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int m = m0 + wm * 64 + 16 * t + ln;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 64 + 16 * j + 4 * lg;
            cca::fbuf_store_x2(Ob, cca::cvt_pk_bf16(acc[t][j][0], acc[t][j][1]), cca::cvt_pk_bf16(acc[t][j][2], acc[t][j][3]),
                               (m < M && n < N) ? (m * ldo + n) * 2 : kOobOffset, 0);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The stacked operands of one module application from the six parameter tensors (bf16, or fp32 = what autocast keeps: rounded to
// nearest even): w (N, C) = [wq; wk; wv], wt (C, N) = its transpose, b (N) fp32 = [bq; bk; bv].  One thread per weight element
// (1.3 MB at C = 512); packed on every forward, no cache (a cache keyed on tensor versions goes stale under ``p.data`` updates).
// ---------------------------------------------------------------------------------------------------------------
template <typename PT>
__device__ __forceinline__ float param_f32(const void *p, long i) {
    return cca::load_f32(static_cast<const PT *>(p) + i);
}

template <typename PT>
__global__ __launch_bounds__(256) void pack_kernel(const void *__restrict__ wq, const void *__restrict__ wk, const void *__restrict__ wv,
                                                   const void *__restrict__ bq, const void *__restrict__ bk, const void *__restrict__ bv,
                                                   bf16_t *__restrict__ w, bf16_t *__restrict__ wt, float *__restrict__ b, int C, int Cq) {
    const int N = 2 * Cq + C;
    const long items = (long)N * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (long)gridDim.x * blockDim.x) {
        const int n = (int)(i / C), c = (int)(i - (long)n * C);
        const void *src = n < Cq ? wq : n < 2 * Cq ? wk : wv;
        const int r = n < Cq ? n : n < 2 * Cq ? n - Cq : n - 2 * Cq;
        bf16_t v;
        cca::store_f32(&v, param_f32<PT>(src, (long)r * C + c));              // (a bf16 value converts to itself)
        w[i] = v;
        wt[(long)c * N + n] = v;
        if (c == 0) b[n] = param_f32<PT>(n < Cq ? bq : n < 2 * Cq ? bk : bv, r);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// db[n] = sum_m D[m][n]: the bias gradients.  The rows are cut into S slabs; workgroup (column group, slab) = 64 column quads x 4
// row phases: a thread adds its phase's rows of four neighbouring columns (one 8-byte load per row) in double, the four phases
// are added in phase order through LDS, and the slab's partial goes to ``part`` (S, N) as double.  colsum_finish_kernel -- ONE
// workgroup -- then adds the S partials of every column in slab order and rounds once to fp32.  Fixed order throughout, no atomics.
// ---------------------------------------------------------------------------------------------------------------
constexpr int CS_QUADS = 64, CS_PHASES = 4, CS_THREADS = CS_QUADS * CS_PHASES, CS_COLS = 4 * CS_QUADS;

__global__ __launch_bounds__(CS_THREADS) void colsum_slab_kernel(const bf16_t *__restrict__ D, double *__restrict__ part, int M, int N,
                                                                  int ldd, int slab) {
    __shared__ double red[CS_PHASES][CS_COLS];
    CCA_LDS_REGISTER(red);
    const int tid = threadIdx.x, qd = tid & (CS_QUADS - 1), ph = tid / CS_QUADS;
    const int n = (int)blockIdx.x * CS_COLS + 4 * qd, sl = (int)blockIdx.y;
    const int r0 = sl * slab, r1 = r0 + slab < M ? r0 + slab : M;
    const FBuf Db = cca::make_fbuf(reinterpret_cast<const float *>(D), ((size_t)(M - 1) * ldd + N) * 2);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (n < N) {
#pragma unroll 4
        for (int r = r0 + ph; r < r1; r += CS_PHASES) {
            const u32x2v v = fbuf_load_x2(Db, (r * ldd + n) * 2, 0);
            s[0] += (double)__builtin_bit_cast(float, v[0] << 16);
            s[1] += (double)__builtin_bit_cast(float, v[0] & 0xffff0000u);
            s[2] += (double)__builtin_bit_cast(float, v[1] << 16);
            s[3] += (double)__builtin_bit_cast(float, v[1] & 0xffff0000u);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[ph][4 * qd + e] = s[e];
    __syncthreads();
    if (ph == 0 && n < N) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double t = red[0][4 * qd + e];
#pragma unroll
            for (int p = 1; p < CS_PHASES; ++p) t += red[p][4 * qd + e];
            part[(long)sl * N + n + e] = t;
        }
    }
}

constexpr int CF_THREADS = 1024;

__global__ __launch_bounds__(CF_THREADS) void colsum_finish_kernel(const double *__restrict__ part, float *__restrict__ db, int N, int S) {
    for (int n = threadIdx.x; n < N; n += CF_THREADS) {
        double t = 0.0;
        for (int s = 0; s < S; ++s) t += part[(long)s * N + n];
        db[n] = (float)t;
    }
}

}  // namespace proj
