// conv3_kernels.hpp -- the kernels of libccnet_conv3.so: the 3x3, stride-1, dilated convolution (padding = dilation) on bf16
// channels_last activations as an implicit GEMM with K = 9 C.
//
//     out[r][n] = bf16_rne( sum_t sum_c a[src(r,t)][c] * wt[n][t K + c] + bias[n] + add[r][n] )
//
//         r        the B H W pixels of whole images, pixel-major: r = (b H + h) W + w
//         t        the tap 3 (ky + 1) + (kx + 1), ky, kx in {-1, 0, 1}
//         src(r,t) the pixel (h + ky d, w + kx d) of the same image; zero when it lies outside the image
//         a        (B H W, K) bf16, row stride lda          wt (N, 9 K) bf16, contiguous
//
// conv3_bf16_kernel is csrc_proj/proj_kernels.hpp's gemm_bf16_kernel (which is csrc/cca_gemm.hpp's proj_gemm_kernel on plain bf16
// operands) with another FILL.  Geometry, stages, loop and waits are that kernel's: workgroup = 256 x 128 outputs, 8 wavefronts of
// 64 x 64 (4 x 4 MFMA tiles, v_mfma_f32_16x16x32_bf16), k steps of 64, T16 row tiles moved by LDS-DMA in 1 KiB pieces, three LDS
// stages of 48 KiB, the register ping-pong over two half steps with the stage barrier between them, swapped MFMA operands, the
// accumulators started from bias + addend, one rounding, 8-byte stores.  The k steps run tap by tap: nkt = ceil(K / 64) steps per
// tap, 9 nkt in all; a k step never straddles two taps (a K that is no multiple of 64 ends every tap with a partial step whose
// chunks past K are fetched out of range = zeros, for BOTH operands: KTAIL).  What changes from tap to tap is one scalar, the byte
// displacement ((ky d) W + kx d) lda 2 of the A rows, and which of a lane's four A rows are fetched at all: bit t of okm[p] says
// whether src(row p, t) is inside the image, computed once per lane from (h, w) of its rows; a row whose source is outside is
// fetched at kOobOffset = zeros, exactly as the K tail is.  A tap never reads across an image boundary or a row wrap, because
// the test is on (h, w), not on the row index.
//
// conv3_wgrad_kernel is csrc/cca_gemm.hpp's proj_wgrad_kernel with the tap as one more grid axis:
//
//     part[s][t][n][c] = sum over the rows r of slab s of dy[r][n] * x[src(r,t)][c]
//
// x's row offsets are shifted by the tap's displacement and dead where src is outside the image (the `dead` rule that kernel has
// for rows past its slab).  wgrad_finish_kernel adds the S partials in slab order and writes the parameter's own layout.
#pragma once
#include "cca_gemm.hpp"

#include <conv3_platform.hpp>

namespace conv3 {

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
using cca::PW_BC;
using cca::PW_BN;
using cca::PW_NT;
using cca::PW_TILE;
using cca::T16_PIECE;
using cca::u32x4;

constexpr int kTaps = 9;

struct ConvJob {
    const bf16_t *A, *Wt;         // (M, lda) rows; (N, 9 K) contiguous
    const float *bias;            // (N) or null
    const bf16_t *add;            // (M, ldadd) or null
    bf16_t *out;
    int M, N, K, lda, ldadd, ldo; // M = B H W
    int H, W, d;                  // d <= max(H, W): a larger dilation reaches no pixel and is clamped by the entry point
};

template <bool KTAIL>
__global__ __launch_bounds__(PG_THREADS, 1) void conv3_bf16_kernel(const ConvJob job) {
    __shared__ __attribute__((aligned(16))) float lds[PG_NBUF * PG_STAGE];
    CCA_LDS_REGISTER(lds);
    const int M = job.M, N = job.N, K = job.K, lda = job.lda, ldw = kTaps * job.K, ldo = job.ldo, ldadd = job.ldadd;
    const int ntm = (M + PG_BM - 1) / PG_BM, ntn = (N + PG_BN - 1) / PG_BN;
    const int tl = cca::xcd_logical_id((int)blockIdx.x, (int)gridDim.x);
    // the axis with FEWER tiles runs fastest: the workgroups that share a tile of the other (streamed) operand are neighbours
    const int m0 = (ntn <= ntm ? tl / ntn : tl % ntm) * PG_BM, n0 = (ntn <= ntm ? tl % ntn : tl / ntm) * PG_BN;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = cca::uniform(tid >> 6);
    const int ln = lane & 15, lg = lane >> 4;
    const int wm = wv >> 1, wn = wv & 1;                                       // this wavefront: rows wm * 64 .., columns wn * 64 ..
    const float *bias = job.bias;
    const FBuf Ab = cca::make_fbuf(reinterpret_cast<const float *>(job.A), ((size_t)(M - 1) * lda + K) * 2);
    const FBuf Wb = cca::make_fbuf(reinterpret_cast<const float *>(job.Wt), (size_t)N * ldw * 2);
    const FBuf Ob = cca::make_fbuf(reinterpret_cast<const float *>(job.out), ((size_t)(M - 1) * ldo + N) * 2);
    const FBuf Cb = job.add ? cca::make_fbuf(reinterpret_cast<const float *>(job.add), ((size_t)(M - 1) * ldadd + N) * 2) : Ob;
    const int nkt = (K + PG_BK - 1) / PG_BK, nk = kTaps * nkt;                 // k steps per tap, and in all (>= 9)

    // fill: wavefront wv moves A pieces wv, wv + 8, .. and Wt pieces wv, wv + 8; lane = (row lane >> 3 of the piece, LDS chunk
    // slot lane & 7), which holds the row's 16-byte k chunk slot ^ row (t16_byte<false>).  okm[p]: bit t = tap t's source pixel of
    // A row p lies inside the image (rows past M: no bit; they are computed on zeros and never stored)
    int offa[PG_NPA], offb[PG_NPB], okm[PG_NPA];
    {
        const int pr = lane >> 3, q = (lane & 7) ^ pr;
        const int H = job.H, W = job.W, d = job.d, HW = H * W;
#pragma unroll
        for (int p = 0; p < PG_NPA; ++p) {
            const int r = m0 + 8 * (wv + PG_WAVES * p) + pr;
            offa[p] = ((r < M ? r : M - 1) * lda + 8 * q) * 2;
            const int pix = r % HW, h = pix / W, w = pix - h * W;
            int m = 0;
#pragma unroll
            for (int t = 0; t < kTaps; ++t) {
                const int y = h + (t / 3 - 1) * d, x = w + (t % 3 - 1) * d;
                m |= ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? 1 << t : 0;
            }
            okm[p] = r < M ? m : 0;
        }
#pragma unroll
        for (int p = 0; p < PG_NPB; ++p) {
            const int r = n0 + 8 * (wv + PG_WAVES * p) + pr;
            offb[p] = ((r < N ? r : N - 1) * ldw + 8 * q) * 2;
        }
    }
    const int kq = 8 * ((lane & 7) ^ (lane >> 3));                             // first k of this lane's chunk within a stage
    // the stage the NEXT fill belongs to: tap ftap, k step fkt of the tap, the tap's byte displacement of the A rows (uniform)
    int ftap = 0, fkt = 0, fdisp = 0;
    auto tap_disp = [&](int t) {
        return (int)(((long)((t / 3 - 1) * job.d) * job.W + (t % 3 - 1) * job.d) * lda * 2);
    };
    fdisp = tap_disp(0);
    auto piece = [&](int slot, int i) {                                        // fill instruction i of PG_NPW (A pieces first)
        float *as = lds + slot * PG_STAGE + wv * T16_PIECE;
        // (KTAIL, a K that is no multiple of 64: chunks past the end of the tap are fetched out of range = zeros)
        const bool tail = KTAIL && fkt * PG_BK + kq >= K;
        const int koff = fkt * PG_BK * 2;
        if (i < PG_NPA) {
            const bool dead = tail || !((okm[i] >> ftap) & 1);                  // (the source pixel is outside the image: zeros)
            cca::fbuf_load_to_lds_x4_uncounted(Ab, as + PG_WAVES * i * T16_PIECE, dead ? kOobOffset : offa[i] + fdisp + koff);
        } else {
            cca::fbuf_load_to_lds_x4_uncounted(Wb, as + (PG_APIECES + PG_WAVES * (i - PG_NPA)) * T16_PIECE,
                                               tail ? kOobOffset : offb[i - PG_NPA] + ftap * K * 2 + koff);
        }
    };
    auto advance = [&]() {                                                     // the fill state moves on by one k step
        if (++fkt == nkt) {
            fkt = 0;
            ++ftap;
            fdisp = tap_disp(ftap);
        }
    };
    auto issue = [&](int slot) {
#pragma unroll
        for (int i = 0; i < PG_NPW; ++i) piece(slot, i);
        advance();
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

    issue(0);                                        // (nk >= 9: the first three stages always exist)
    issue(1);
    issue(2);
    stage_barrier<2 * PG_NPW>();            // stage 0 landed
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
    do {                                            // (nk >= 9; no path skips the loop with reads in flight)
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
            if (it + 2 < nk) stage_barrier<PG_NPW>();
            else             stage_barrier<0>();
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
                    if (fill) piece(slot, 4 * t + j);
                    cca::sched_fence();
                }
            }
        cca::sched_fence();
        advance();                                  // (scalar; past the last fill it names stages nobody fetches)
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
// Both packs of the parameter (Cout, Cin, 3, 3), bf16 (copied) or fp32 (rounded to nearest even, what autocast keeps), one thread
// per element: fwd[n][t Cin + c] = w[n][c][t], adj[c][t Cout + n] = w[n][c][8 - t] (the taps mirrored, the channels transposed:
// the input gradient is the same correlation of dy with that operand).  Packed on every forward, no cache.
// ---------------------------------------------------------------------------------------------------------------
template <typename PT>
__global__ __launch_bounds__(256) void pack_kernel(const void *__restrict__ weight, bf16_t *__restrict__ fwd, bf16_t *__restrict__ adj,
                                                   int Cout, int Cin) {
    const long items = (long)Cout * Cin * kTaps;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (long)gridDim.x * blockDim.x) {
        const long nc = i / kTaps;
        const int t = (int)(i - nc * kTaps), n = (int)(nc / Cin), c = (int)(nc - (long)n * Cin);
        bf16_t v;
        cca::store_f32(&v, cca::load_f32(static_cast<const PT *>(weight) + i));      // (a bf16 value converts to itself)
        fwd[((long)n * kTaps + t) * Cin + c] = v;
        adj[((long)c * kTaps + (kTaps - 1 - t)) * Cout + n] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The weight gradient: proj_wgrad_kernel (csrc/cca_gemm.hpp) with the tap as one more grid axis.  Workgroup (slab, tile, tap) --
// the nine taps of a tile neighbours: they read the same dy tile and x rows a few image rows apart -- contracts the slab's rows
// of dy (R, N) with the SHIFTED rows of x (R, C): a stage is 64 rows; the x row of a lane is fetched at its own offset plus the
// tap's displacement, or out of range = zeros where the row is past the slab or its source pixel outside the image.  (h, w) of a
// lane's row is recomputed per stage (two integer divisions per lane and 64 rows, next to 32 MFMAs).
// ---------------------------------------------------------------------------------------------------------------
struct WgradJob {
    const bf16_t *D, *X;          // dy (R, ldd), x (R, ldx)
    float *part;                  // (S, 9, N, C)
    int R, N, C, ldd, ldx, S, slab;   // slab = rows per slab, a multiple of 64
    int H, W, d;
};

__global__ __launch_bounds__(PG_THREADS, 1) void conv3_wgrad_kernel(const WgradJob job) {
    __shared__ __attribute__((aligned(16))) float lds[PG_NBUF * PG_STAGE];
    CCA_LDS_REGISTER(lds);
    const int N = job.N, C = job.C, ldd = job.ldd, ldx = job.ldx, H = job.H, W = job.W, HW = H * W;
    const int ntc = (C + PW_BC - 1) / PW_BC, ntn = (N + PW_BN - 1) / PW_BN;
    const int lid = cca::xcd_logical_id((int)blockIdx.x, (int)gridDim.x);
    const int tap = lid % kTaps, st_ = lid / kTaps;
    const int sl = st_ / (ntn * ntc), tl = st_ - sl * (ntn * ntc);
    const int n0 = (tl / ntc) * PW_BN, c0 = (tl % ntc) * PW_BC;
    // (a forced slab count may leave slabs wholly past R: their first row is clamped to R, so no row index or offset leaves int)
    const long first = (long)sl * job.slab;
    const int r0 = first < job.R ? (int)first : job.R, r1 = (long)r0 + job.slab < job.R ? r0 + job.slab : job.R;
    const int nk = r1 > r0 ? (r1 - r0 + PG_BK - 1) / PG_BK : 0;
    const int sy = (tap / 3 - 1) * job.d, sx = (tap % 3 - 1) * job.d;                // the tap's shift in image rows and columns
    const int xshift = (int)(((long)sy * W + sx) * ldx * 2);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = cca::uniform(tid >> 6);
    const int ln = lane & 15, lg = lane >> 4;
    const int wn = wv >> 2, wc = wv & 3;                                             // this wavefront: n columns 64 wn .., c columns 64 wc ..
    const FBuf Db = cca::make_fbuf(reinterpret_cast<const float *>(job.D), ((size_t)(job.R - 1) * ldd + N) * 2);
    const FBuf Xb = cca::make_fbuf(reinterpret_cast<const float *>(job.X), ((size_t)(job.R - 1) * ldx + C) * 2);
    const FBuf Ob = cca::make_fbuf(job.part + ((size_t)sl * kTaps + tap) * N * C, (size_t)N * C * sizeof(float));

    // fill: wavefront wv moves piece wv (rows 8 wv .. + 7 of the stage) of all six tiles; lane = (row lane >> 3, LDS chunk slot
    // lane & 7), which holds the row's 16-byte channel chunk q (t16_dma_piece, FLIP layout)
    const int pr = lane >> 3, q = (lane & 7) ^ pr ^ ((wv & 1) << 2), rs = 8 * wv + pr;       // row of this lane within a stage
    int off[PW_NT];
#pragma unroll
    for (int t = 0; t < PW_NT; ++t) {
        const bool isd = t < PW_BN / 64;
        const int ch = (isd ? n0 + 64 * t : c0 + 64 * (t - PW_BN / 64)) + 8 * q;
        // (columns past the matrix, and rows past it: zeros; a row inside it has an offset below 2^31 by the entry point's check)
        off[t] = (ch < (isd ? N : C) && r0 + rs < job.R) ? ((r0 + rs) * (isd ? ldd : ldx) + ch) * 2 : kOobOffset;
    }
    auto issue = [&](int it, int slot) {
        float *st = lds + slot * PG_STAGE + wv * T16_PIECE;
        const int r = r0 + it * PG_BK + rs;
        const bool dead = r >= r1;                                                               // rows past the slab: zeros
        const int pix = r % HW, h = pix / W, w = pix - h * W;
        // (x alone: the source pixel of this row under the tap is outside the image -- zeros, whatever dy holds)
        const bool xdead = dead || (unsigned)(h + sy) >= (unsigned)H || (unsigned)(w + sx) >= (unsigned)W;
#pragma unroll
        for (int t = 0; t < PW_NT; ++t) {
            const bool isd = t < PW_BN / 64;
            const int o = ((isd ? dead : xdead) || off[t] == kOobOffset) ? kOobOffset
                                                                          : off[t] + it * PG_BK * (isd ? ldd : ldx) * 2 + (isd ? 0 : xshift);
            cca::fbuf_load_to_lds_x4_uncounted(isd ? Db : Xb, st + t * PW_TILE, o);
        }
    };

    // lane (ln, lg) of tile (a, b) holds c = c0 + 64 wc + 16 b + 4 lg .. + 3 of n = n0 + 64 wn + 16 a + ln
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (nk > 0) issue(0, 0);
    if (nk > 1) issue(1, 1);
    if (nk > 2) issue(2, 2);
    if (nk > 2)       stage_barrier<2 * PW_NT>();                            // stage 0 landed
    else if (nk > 1)  stage_barrier<PW_NT>();
    else              stage_barrier<0>();
    int slot = 0;
    for (int it = 0; it < nk; ++it) {
        const float *dt = lds + slot * PG_STAGE + wn * PW_TILE, *xt = lds + slot * PG_STAGE + (PW_BN / 64 + wc) * PW_TILE;
        u32x4 df[4], xf[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) { df[a] = cca::t16_frag(dt, 0, a, lane); xf[a] = cca::t16_frag(xt, 0, a, lane); }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = cca::mfma_bf16_16x16x32(xf[b], df[a], acc[a][b]);
#pragma unroll
        for (int a = 0; a < 4; ++a) { df[a] = cca::t16_frag(dt, 1, a, lane); xf[a] = cca::t16_frag(xt, 1, a, lane); }
        if (it + 1 < nk) {
            // stage it + 1 landed and every wavefront holds the rest of stage `it` in registers (the barrier drains its LDS reads):
            // the slot takes stage it + 3 at once, the fill of stage it + 2 stays in flight
            if (it + 2 < nk) stage_barrier<PW_NT>();
            else             stage_barrier<0>();
            if (it + 3 < nk) issue(it + 3, slot);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = cca::mfma_bf16_16x16x32(xf[b], df[a], acc[a][b]);
        slot = slot == PG_NBUF - 1 ? 0 : slot + 1;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int n = n0 + 64 * wn + 16 * a + ln;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int c = c0 + 64 * wc + 16 * b + 4 * lg;
            // (C % 8 == 0: the four channels are inside the matrix together or not at all)
            cca::fbuf_store_x4(Ob, acc[a][b], (n < N && c < C) ? (n * C + c) * 4 : kOobOffset, 0);
        }
    }
}

// dw[n][c][t] = sum_s part[s][t][n][c]: one thread per (n, c), the S partials of each tap added in slab order in fp32, the nine
// results written side by side in the parameter's layout; OT = bf16_t rounds once to nearest even, float writes the sums as they are
template <typename OT>
__global__ __launch_bounds__(256) void wgrad_finish_kernel(const float *__restrict__ part, OT *__restrict__ dw, long NC, int S) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < NC; i += (long)gridDim.x * blockDim.x) {
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
            float v = part[(long)t * NC + i];
            for (int s = 1; s < S; ++s) v += part[((long)s * kTaps + t) * NC + i];
            cca::store_f32(dw + i * kTaps + t, v);
        }
    }
}

}  // namespace conv3
