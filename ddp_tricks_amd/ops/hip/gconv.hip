// gconv.hip — grouped 3x3 convolution on MFMA for gfx950: forward, dgrad,
// wgrad and the weight pack.
//
// Scope: groups > 1, C_in == C_out == C, C % 64 == 0, Cg = C / groups in
// {4, 8, 16, 32, 64}; 3x3, dilation 1, one stride (1 or 2) and one padding
// (0 or 1) for both dims; bf16 channels_last activations, fp32 master weight
// [C, Cg, 3, 3], optional fp32 bias.
//
// The unit of work is a 64-channel SPAN.  Cg == Kg, so input channels
// [64j, 64j + 64) feed exactly output channels [64j, 64j + 64) for every Cg
// in scope: per tap the A operand of a span is 128 B contiguous per pixel and
// the B operand a 64x64 block-diagonal matrix.  An output sub-tile of 16
// channels needs only the KW = max(16, Cg) input channels of the groups it
// intersects; the other K segments of the staged tile are never read for it.
// KW = 16, 32, 64 are the three instantiations for the five Cg.  At Cg = 4 / 8
// the 16x16 diagonal block carries zeros inside (4x / 2x wasted MFMA).
//
// A grouped conv's arithmetic intensity is 1/groups of a dense conv's, so the
// kernels are laid out to stream x and y (dy and dx, dy and x) once from HBM;
// the nine taps re-read the same pixels from L2.  Bytes at 8 TB/s against the
// MFMA work including the zero fill at a dense rate of 1.2 PFLOP/s (the
// 16x16x32 instruction; the 16-deep one KW = 16 uses runs at half of it), at
// B = 256, pad 1, forward:
//     C    H  s  Cg   HBM MB   HBM us   GFLOP(fill)  MFMA us
//    128  56  1   4    411.0    51.4      29.6        49.3 (16-deep)
//    256  56  2   8    256.9    32.1      14.8        24.7 (16-deep)
//    256  28  1   8    205.5    25.7      14.8        24.7 (16-deep)
//    512  28  2  16    128.5    16.1       7.4        12.3 (16-deep)
//    512  14  1  16    102.8    12.8       7.4        12.3 (16-deep)
//   1024  14  2  32     64.2     8.0       7.4         6.2
//   1024   7  1  32     51.4     6.4       7.4         6.2
//   2048   7  1  64    102.8    12.8      29.6        24.7
// The MFMA column is a peak-rate floor; with four waves of a block sharing a
// SIMD's matrix unit in turn with their LDS reads it is not reached, so at
// Cg = 4 / 8 the zero fill may show (docs/KERNELS.md, "Grouped conv").
//
// Data movement: operands are staged by __builtin_amdgcn_global_load_lds
// (16 B per lane, no VGPR round trip).  The DMA writes lane-linear, so the
// bank swizzle (16 B segment ^ (row & 7) on 128 B rows) sits on the per-lane
// SOURCE address and is repeated on the fragment reads, as in k_conv_gemm.
// Lanes whose source is out of range (row past M, padding tap) read a zeroed
// 16 B device buffer; no lane hands the DMA an address outside its tensor.
// Reductions (BN statistics, dw) are fixed-order: per-block slab slots and an
// in-order combine, no atomics; every grid is a function of the shape alone
// (gc_plan, the one place that decides).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <algorithm>
#include <climits>
#include <string>
#include <tuple>
#include "common.h"

typedef short gc_bf16x8 __attribute__((ext_vector_type(8)));
typedef short gc_bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) gc_bf16x4* gc_lds_tr16_ptr;

__device__ __align__(16) unsigned char gc_zero16[16];

constexpr int GC_SPAN = 64;          // channels per span
constexpr int GC_BM = 128;           // forward / dgrad row tile
constexpr int GC_WD = 64;            // wgrad rows (contraction) per tile
constexpr int GC_TILES_PER_BLOCK = 4;     // least wgrad tiles per block
constexpr int GC_WGRAD_MAX_BLOCKS = 2048; // spans * split cap
constexpr int GC_COMBINE_CH = 32;         // stage-1 combine depth
constexpr int GC_COMBINE_DIRECT = 64;     // deeper slabs combine in two stages
constexpr int GC_OFF = -(1 << 30);        // coordinate of a row past M

DEV_INLINE short gc_f2bf_bits(float f) {
    return __builtin_bit_cast(short, (__bf16)f);
}

DEV_INLINE void gc_dma16(unsigned long src, bf16* lds_dst) {
    __builtin_amdgcn_global_load_lds(
        reinterpret_cast<const __attribute__((address_space(1)))
                         unsigned short*>(src),
        (__attribute__((address_space(3))) unsigned short*)lds_dst, 16, 0, 0);
}

// ------------------------------------------------------------- weight pack ---
// fp32 master [C][Cg][3][3] -> two bf16 images [C/64][9][64][64], rounding
// f2us as k_pack_conv_weight.  fwd[j][t][o][i] = w[64j + o][i'][t] where input
// channel 64j + i lies in o's group (i' its index there), else 0.  The dgrad
// image is the same with taps flipped and each block transposed:
// dgr[j][8 - t][i][o] = fwd[j][t][o][i], so the forward kernel over dy with
// that image contracts over the output channels.
__global__ void k_pack_gconv_weight(const float* __restrict__ w, int C, int Cg,
                                    unsigned short* __restrict__ fwd,
                                    unsigned short* __restrict__ dgr) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)C * 9 * GC_SPAN) return;
    const int i = idx & 63, o = (idx >> 6) & 63;
    const int jt = (int)(idx >> 12);
    const int j = jt / 9, t = jt - j * 9;
    const int k = j * GC_SPAN + o;
    const int cin = j * GC_SPAN + i;
    const int c = cin - (k / Cg) * Cg;
    unsigned short v = 0;
    if (c >= 0 && c < Cg) v = f2us(w[((long)k * Cg + c) * 9 + t]);
    fwd[idx] = v;
    dgr[(((long)j * 9 + (8 - t)) * GC_SPAN + i) * GC_SPAN + o] = v;
}

// ------------------------------------------------------ forward and dgrad ---
struct GcShape {
    int N, C;
    int Hs, Ws;         // the tensor read (x forward, dy dgrad)
    int Ho, Wo;         // the tensor written (y forward, dx dgrad)
    int sstride, spad;  // output pixel (h, w) reads source (h*sstride - spad
                        // + du, ...) at tap offset (du, dv)
    int cpad;           // CLS: the conv's padding
    int M;              // GEMM rows N * Ho * Wo (not CLS)
};

// One block: rows [128 bx, 128 bx + 128) of span blockIdx.y; four waves of
// 32 rows x 64 channels.  Per tap: A [128][64] and B [64 out][64 in] by DMA,
// one barrier, the MFMAs over the diagonal K segments, one barrier.  Single
// buffer (24.5 KiB LDS): like k_conv_gemm this kernel hides latency with
// resident blocks, not with a ring.
//
// KW = 16 uses the 16-deep MFMA over one tap: the 32-deep instruction would
// want the second 16 K values from the next tap, i.e. two taps' A tiles
// resident (48 KiB LDS, half the blocks per CU) and an odd ninth tap.
// KW = 32 / 64 use mfma_f32_16x16x32_bf16 inside one tap.
//
// The forward (sstride = stride, spad = pad) and the stride-1 dgrad (over dy,
// dgrad image, spad = 2 - pad) walk all nine taps at offsets (r, s).  CLS is
// the stride-2 dgrad: blockIdx.z is the residue class (a, b) = (h & 1, w & 1)
// of dx, the rows are that class's pixels (h, w) = (2h' + a, 2w' + b), and
// only the taps with a + pad - r and b + pad - s even contribute (1, 2, 2 or
// 4 taps, block-uniform): p = h' + (a + pad - r) / 2.  The four classes tile
// dx, and a pixel no output reads has every tap out of range, so it gets its
// zeros here.
//
// Epilogue: accumulators (+ bias) rounded to bf16 through the A tile's LDS,
// written as 16 B chunks of a row's 128 B.  STATS: per-block sum and sum of
// squares of the pre-rounding values into slab[2][C][gridDim.x] (the layout
// of conv2d_fwd_stats): lane chain over its 8 rows, two shuffles over the
// row quads, the four waves in order through LDS.
template <int KW, bool BIAS, bool STATS, bool CLS>
__global__ __launch_bounds__(256) NO_PK_F32
void k_gconv_fwd(const bf16* __restrict__ src, const bf16* __restrict__ wimg,
                 const float* __restrict__ bias, bf16* __restrict__ out,
                 float* __restrict__ slab, GcShape g) {
    __shared__ __align__(16) bf16 lds_a[GC_BM][GC_SPAN];
    __shared__ __align__(16) bf16 lds_b[GC_SPAN][GC_SPAN];
    __shared__ int opix[GC_BM];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int span = blockIdx.y;
    int ca = 0, cb = 0, Hr = g.Ho, Wr = g.Wo, M = g.M;
    if (CLS) {
        ca = blockIdx.z >> 1; cb = blockIdx.z & 1;
        Hr = (g.Ho - ca + 1) >> 1; Wr = (g.Wo - cb + 1) >> 1;
        M = g.N * Hr * Wr;
    }
    const int m0 = blockIdx.x * GC_BM;
    if (CLS && m0 >= M) return;         // block-uniform, before any barrier

    // staging: wave wid fills 8-row chunks wid + 4i; a lane's row within the
    // chunk and its logical segment are the same in every chunk
    const int srow = lane >> 3;
    const int seg8 = ((lane & 7) ^ srow) * 8;
    int ru[4], rv[4];
    long a_off[4];
    #pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
        const int row = (wid + ci * 4) * 8 + srow;
        const int gm = m0 + row;
        ru[ci] = GC_OFF; rv[ci] = GC_OFF; a_off[ci] = 0;
        int op = -1;
        if (gm < M) {
            const int rem = gm / Wr, rw = gm - rem * Wr;
            const int n = rem / Hr, rh = rem - n * Hr;
            ru[ci] = rh * g.sstride - g.spad;
            rv[ci] = rw * g.sstride - g.spad;
            a_off[ci] = ((((long)n * g.Hs + ru[ci]) * g.Ws + rv[ci]) * g.C
                         + span * GC_SPAN + seg8) * (long)sizeof(bf16);
            op = CLS ? (n * g.Ho + 2 * rh + ca) * g.Wo + 2 * rw + cb : gm;
        }
        if ((lane & 7) == 0) opix[row] = op;
    }
    unsigned long zaddr = reinterpret_cast<unsigned long>(gc_zero16);
    asm volatile("" : "+s"(zaddr));
    const unsigned long b_lane = reinterpret_cast<unsigned long>(wimg)
        + (unsigned long)((((long)span * 9 * GC_SPAN + wid * 8 + srow)
                           * GC_SPAN + seg8) * (long)sizeof(bf16));

    f32x4 acc[2][4] = {};
    const int fr = lane & 15;           // fragment row / column
    const int fk = lane >> 4;           // fragment k block

    auto do_tap = [&](int du, int dv, int ti)
            __attribute__((always_inline)) {
        const unsigned long abase = reinterpret_cast<unsigned long>(src)
            + (unsigned long)(((long)du * g.Ws + dv) * g.C
                              * (long)sizeof(bf16));
        #pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
            const bool ok = (unsigned)(ru[ci] + du) < (unsigned)g.Hs &&
                            (unsigned)(rv[ci] + dv) < (unsigned)g.Ws;
            gc_dma16(ok ? abase + (unsigned long)a_off[ci] : zaddr,
                     &lds_a[(wid + ci * 4) * 8][0]);
        }
        const unsigned long bbase = b_lane
            + (unsigned long)((long)ti * GC_SPAN * GC_SPAN * sizeof(bf16));
        #pragma unroll
        for (int bi = 0; bi < 2; ++bi)
            gc_dma16(bbase + (unsigned long)(bi * 32 * GC_SPAN * sizeof(bf16)),
                     &lds_b[(wid + bi * 4) * 8][0]);
        __syncthreads();   // vmcnt(0) for the in-flight DMA + barrier
        if constexpr (KW == 16) {
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                // channels 16 ni + 4 fk .. + 4: 8 B inside one 16 B segment
                const int seg = 2 * ni + (fk >> 1), sub = (fk & 1) * 4;
                const int brow = ni * 16 + fr;
                const gc_bf16x4 bf = *reinterpret_cast<const gc_bf16x4*>(
                    &lds_b[brow][((seg ^ (brow & 7)) << 3) + sub]);
                #pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    const int arow = wid * 32 + mi * 16 + fr;
                    const gc_bf16x4 af = *reinterpret_cast<const gc_bf16x4*>(
                        &lds_a[arow][((seg ^ (arow & 7)) << 3) + sub]);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
                        af, bf, acc[mi][ni], 0, 0, 0);
                }
            }
        } else {
            // K halves of 32 channels: A fragments are shared by the output
            // tiles that read the half
            gc_bf16x8 af[2][2];
            #pragma unroll
            for (int mi = 0; mi < 2; ++mi)
                #pragma unroll
                for (int kh = 0; kh < 2; ++kh) {
                    const int arow = wid * 32 + mi * 16 + fr;
                    af[mi][kh] = *reinterpret_cast<const gc_bf16x8*>(
                        &lds_a[arow][((kh * 4 + fk) ^ (arow & 7)) << 3]);
                }
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int brow = ni * 16 + fr;
                #pragma unroll
                for (int kh = 0; kh < 2; ++kh) {
                    if (KW == 32 && kh != (ni >> 1)) continue;
                    const gc_bf16x8 bf = *reinterpret_cast<const gc_bf16x8*>(
                        &lds_b[brow][((kh * 4 + fk) ^ (brow & 7)) << 3]);
                    #pragma unroll
                    for (int mi = 0; mi < 2; ++mi)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            af[mi][kh], bf, acc[mi][ni], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    };

    if constexpr (!CLS) {
        for (int r = 0; r < 3; ++r)
            for (int s = 0; s < 3; ++s) do_tap(r, s, r * 3 + s);
    } else {
        for (int r = 0; r < 3; ++r) {
            const int er = ca + g.cpad - r;
            if (er & 1) continue;
            for (int s = 0; s < 3; ++s) {
                const int es = cb + g.cpad - s;
                if (es & 1) continue;
                do_tap(er >> 1, es >> 1, 8 - (r * 3 + s));
            }
        }
    }

    // the loop's last barrier has retired every read of both tiles
    bf16* stage = &lds_a[0][0];                           // [128][64]
    float* red = reinterpret_cast<float*>(&lds_b[0][0]);  // [4][64][2]
    float psum[4] = {}, psq[4] = {};
    #pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int cl = ni * 16 + fr;
        const float badd = BIAS ? bias[span * GC_SPAN + cl] : 0.f;
        #pragma unroll
        for (int mi = 0; mi < 2; ++mi)
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = wid * 32 + mi * 16 + fk * 4 + r;
                const float v = acc[mi][ni][r] + badd;
                if (STATS && m0 + rl < M) {
                    psum[ni] += v;
                    psq[ni] = fmaf(v, v, psq[ni]);
                }
                reinterpret_cast<short*>(stage)[rl * GC_SPAN + cl] =
                    gc_f2bf_bits(v);
            }
    }
    if constexpr (STATS) {
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            float a = psum[ni], b = psq[ni];
            a += __shfl_down(a, 32, 64);
            a += __shfl_down(a, 16, 64);
            b += __shfl_down(b, 32, 64);
            b += __shfl_down(b, 16, 64);
            if (fk == 0) {
                red[(wid * GC_SPAN + ni * 16 + fr) * 2] = a;
                red[(wid * GC_SPAN + ni * 16 + fr) * 2 + 1] = b;
            }
        }
    }
    __syncthreads();
    const int rsub = tid >> 3, csub = (tid & 7) * 8;
    #pragma unroll
    for (int pass = 0; pass < GC_BM / 32; ++pass) {
        const int rl = pass * 32 + rsub;
        const int op = opix[rl];
        if (op >= 0)
            *reinterpret_cast<gc_bf16x8*>(
                &out[(long)op * g.C + span * GC_SPAN + csub]) =
                *reinterpret_cast<const gc_bf16x8*>(
                    &stage[rl * GC_SPAN + csub]);
    }
    if constexpr (STATS) {
        if (tid < GC_SPAN) {
            float a = 0.f, b = 0.f;
            #pragma unroll
            for (int w = 0; w < 4; ++w) {
                a += red[(w * GC_SPAN + tid) * 2];
                b += red[(w * GC_SPAN + tid) * 2 + 1];
            }
            const long col = span * GC_SPAN + tid;
            slab[col * gridDim.x + blockIdx.x] = a;
            slab[((long)g.C + col) * gridDim.x + blockIdx.x] = b;
        }
    }
}

// -------------------------------------------------------------------- wgrad ---
struct GwShape {
    int N, C, Cg;
    int H, W, P, Q;
    int stride, pad;
    int M, tiles;       // rows N * P * Q, 64-row tiles
    FastDiv fdQ, fdP;
};

// dw[k][c][r][s] = sum over m of dy[m][k] * x[m @ (r, s)][c], c in k's group.
// Block (span, split) takes the 64-row tiles split, split + S, ...  Both
// operands are m-major in memory, so the images are the natural [m][64]
// filled by DMA and the fragments (m contiguous per lane) come from the
// transposed read ds_read_b64_tr_b16: in a 16-lane group lane g addresses
// img[R + (g >> 2)][col + (g & 3) * 4] and receives img[R + j][col + g],
// j = 0 .. 3; a fragment is two reads 4 rows apart.  The transpose is over
// the data the 16 lanes load, so each lane's address carries its own row's
// swizzle.  The read needs EXEC all ones: nothing lane-divergent encloses
// the read + MFMA block.
//
// Per tile the dy image is staged once and its fragments kept in registers;
// the x image is staged three taps (one kernel row r) per barrier pair, so a
// pair covers 6 KW/16 MFMAs per wave, not 2 KW/16.  LDS 32 KiB.
// Wave w owns output channels [16w, 16w + 16) of the span and the KW/16
// input tiles of their KW block, for all 9 taps: 9 KW/16 f32x4 accumulators
// (36 at KW = 64; the resource report in docs/KERNELS.md shows 2 waves/SIMD,
// so the taps stay in one block).
// The partials go to slab[split][C][Cg][9]; at KW = 16 a 16x16 tile spans
// 16 / Cg groups and only its diagonal Cg x Cg blocks are stored.
template <int KW>
__global__ __launch_bounds__(256) NO_PK_F32
void k_gconv_wgrad(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                   float* __restrict__ slab, GwShape g) {
    __shared__ __align__(16) bf16 img_dy[GC_WD][GC_SPAN];
    __shared__ __align__(16) bf16 img_x[3][GC_WD][GC_SPAN];
    constexpr int NI = KW / 16;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int span = blockIdx.x, split = blockIdx.y, S = gridDim.y;
    const int srow = lane >> 3;
    const int seg8 = ((lane & 7) ^ srow) * 8;
    unsigned long zaddr = reinterpret_cast<unsigned long>(gc_zero16);
    asm volatile("" : "+s"(zaddr));

    // fragment reads: element offsets inside a 32-row step, low and high half
    const int fg = lane & 15, fk = lane >> 4;
    const int frow = fk * 8 + (fg >> 2);            // (frow & 7) == fg >> 2
    auto frag_off = [&](int tile16, int hi)
            __attribute__((always_inline)) {
        const int row = frow + hi * 4;
        const int seg = tile16 * 2 + ((fg & 3) >> 1);
        return row * GC_SPAN + ((seg ^ (row & 7)) << 3) + (fg & 1) * 4;
    };
    auto frag = [&](const bf16* img, int ks, int tile16)
            __attribute__((always_inline)) {
        gc_bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (gc_lds_tr16_ptr)(img + ks * GC_SPAN + frag_off(tile16, 0)));
        gc_bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (gc_lds_tr16_ptr)(img + ks * GC_SPAN + frag_off(tile16, 1)));
        return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    };
    const int in0 = (wid * 16 / KW) * NI;           // first input tile

    f32x4 acc[9][NI] = {};
    for (int t = split; t < g.tiles; t += S) {
        int h0[2], w0[2];
        long xoff[2];
        #pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int gm = t * GC_WD + (wid + 4 * i) * 8 + srow;
            const bool ok = gm < g.M;
            const unsigned rem = fd_div((unsigned)gm, g.fdQ);
            const int q = (int)fd_mod((unsigned)gm, g.fdQ, rem);
            const unsigned n = fd_div(rem, g.fdP);
            const int p = (int)fd_mod(rem, g.fdP, n);
            h0[i] = ok ? p * g.stride - g.pad : GC_OFF;
            w0[i] = ok ? q * g.stride - g.pad : GC_OFF;
            xoff[i] = ok ? ((((long)n * g.H + h0[i]) * g.W + w0[i]) * g.C
                            + span * GC_SPAN + seg8) * (long)sizeof(bf16)
                         : 0;
            const unsigned long a = reinterpret_cast<unsigned long>(dy)
                + (unsigned long)(((long)gm * g.C + span * GC_SPAN + seg8)
                                  * (long)sizeof(bf16));
            gc_dma16(ok ? a : zaddr, &img_dy[(wid + 4 * i) * 8][0]);
        }
        gc_bf16x8 af[2];
        #pragma unroll
        for (int r = 0; r < 3; ++r) {
            #pragma unroll
            for (int s = 0; s < 3; ++s) {
                const unsigned long xb = reinterpret_cast<unsigned long>(x)
                    + (unsigned long)(((long)r * g.W + s) * g.C
                                      * (long)sizeof(bf16));
                #pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const bool ok =
                        (unsigned)(h0[i] + r) < (unsigned)g.H &&
                        (unsigned)(w0[i] + s) < (unsigned)g.W;
                    gc_dma16(ok ? xb + (unsigned long)xoff[i] : zaddr,
                             &img_x[s][(wid + 4 * i) * 8][0]);
                }
            }
            __syncthreads();   // vmcnt(0) for the in-flight DMA + barrier
            if (r == 0) {
                af[0] = frag(&img_dy[0][0], 0, wid);
                af[1] = frag(&img_dy[0][0], 32, wid);
            }
            #pragma unroll
            for (int s = 0; s < 3; ++s)
                #pragma unroll
                for (int ks = 0; ks < 2; ++ks)
                    #pragma unroll
                    for (int ni = 0; ni < NI; ++ni) {
                        const gc_bf16x8 bf = frag(&img_x[s][0][0], ks * 32,
                                                  in0 + ni);
                        acc[r * 3 + s][ni] =
                            __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                af[ks], bf, acc[r * 3 + s][ni], 0, 0, 0);
                    }
            __syncthreads();
        }
    }

    // acc[.][ni][j]: output channel 16 wid + 4 fk + j, input channel
    // 16 (in0 + ni) + fg of the span
    #pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        const int ci = (in0 + ni) * 16 + fg;
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ko = wid * 16 + fk * 4 + j;
            const int grp = ko / g.Cg;
            const int c = ci - grp * g.Cg;
            if (c < 0 || c >= g.Cg) continue;
            float* dst = slab + (((long)split * g.C + span * GC_SPAN + ko)
                                 * g.Cg + c) * 9;
            #pragma unroll
            for (int t9 = 0; t9 < 9; ++t9) dst[t9] = acc[t9][ni][j];
        }
    }
}

// out[y][i] = slab[y*CH .. min(S, y*CH + CH))[i] summed in fixed order; the
// slab's [C][Cg][9] is dw's own layout, so the last (or only) stage writes dw.
// Two chains, even / odd slices, keep two loads in flight.
__global__ void k_gconv_wgrad_combine(const float* __restrict__ slab, int S,
                                      int CH, long total,
                                      float* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int s0 = blockIdx.y * CH;
    const int se = min(S, s0 + CH);
    float v0 = 0.f, v1 = 0.f;
    int s = s0;
    for (; s + 1 < se; s += 2) {
        v0 += slab[(long)s * total + i];
        v1 += slab[(long)(s + 1) * total + i];
    }
    if (s < se) v0 += slab[(long)s * total + i];
    out[(long)blockIdx.y * total + i] = v0 + v1;
}

// -------------------------------------------------------------------- hosts ---

enum GcOp { GC_FWD = 0, GC_DGRAD = 1, GC_WGRAD = 2 };

struct GcPlan {
    std::string name;
    int kw, row_tile;
    long gx, gy, gz;
    int split;
    bool cls;
    GcShape s;
    GwShape w;
};

static void gc_check_scope(long C, long groups, long stride, long pad) {
    TORCH_CHECK(groups > 1 && C >= 64 && C % 64 == 0 && C % groups == 0,
                "gconv2d: needs groups > 1 and C_in == C_out == C with "
                "C % 64 == 0; got C=", C, " groups=", groups);
    const long Cg = C / groups;
    TORCH_CHECK(Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32 || Cg == 64,
                "gconv2d: C / groups must be 4, 8, 16, 32 or 64; got ", Cg);
    TORCH_CHECK((stride == 1 || stride == 2) && (pad == 0 || pad == 1),
                "gconv2d: stride must be 1 or 2 and padding 0 or 1; got "
                "stride=", stride, " pad=", pad);
}

// The one place that decides instantiation, row tile, grid and split; pure
// host arithmetic.  (N, C, H, W) is always the conv's input x.
//   * KW = max(16, Cg).
//   * fwd / dgrad: 128-row tiles on grid.x, spans on grid.y; the stride-2
//     dgrad puts the four residue classes on grid.z and sizes grid.x for the
//     largest (class (0, 0)); overhanging blocks of the others exit.
//   * wgrad: spans on grid.x, the split S on grid.y.  S is the smallest of
//     tiles / 4 (a block's 9 KW/16 x 4 scattered stores per lane want some
//     tiles to amortise over), 2048 / spans (blocks), and M / (36 Cg): the
//     slab is S C Cg 36 B against 4 M C B of dy and x, so this keeps the slab
//     under a quarter of the operand traffic where C is wide and M small.
static GcPlan gc_plan(GcOp op, long N, long C, long H, long W, long groups,
                      long stride, long pad) {
    gc_check_scope(C, groups, stride, pad);
    TORCH_CHECK(N >= 1 && H + 2 * pad >= 3 && W + 2 * pad >= 3,
                "gconv2d: input smaller than the 3x3 window");
    TORCH_CHECK(N * H * W < INT_MAX / 2 && N * H * W * C < (1L << 40),
                "gconv2d: index range");
    const long P = (H + 2 * pad - 3) / stride + 1;
    const long Q = (W + 2 * pad - 3) / stride + 1;
    const long Cg = C / groups;
    GcPlan pl;
    pl.kw = (int)std::max<long>(16, Cg);
    pl.cls = false;
    pl.split = 1;
    pl.gz = 1;
    pl.s = GcShape{};
    pl.w = GwShape{};
    const std::string kw = "_kw" + std::to_string(pl.kw);
    if (op == GC_WGRAD) {
        GwShape& w = pl.w;
        w.N = (int)N; w.C = (int)C; w.Cg = (int)Cg;
        w.H = (int)H; w.W = (int)W; w.P = (int)P; w.Q = (int)Q;
        w.stride = (int)stride; w.pad = (int)pad;
        w.M = (int)(N * P * Q);
        w.tiles = ceil_div_i(w.M, GC_WD);
        w.fdQ.init((unsigned)Q); w.fdP.init((unsigned)P);
        const long spans = C / GC_SPAN;
        long S = std::min<long>(ceil_div_i(w.tiles, GC_TILES_PER_BLOCK),
                                GC_WGRAD_MAX_BLOCKS / spans);
        S = std::min<long>(S, w.M / (36 * Cg));
        S = std::max<long>(1, std::min<long>(S, w.tiles));
        pl.split = (int)S;
        pl.row_tile = GC_WD;
        pl.gx = spans; pl.gy = S;
        pl.name = "wgrad" + kw;
        return pl;
    }
    GcShape& s = pl.s;
    s.N = (int)N; s.C = (int)C;
    s.cpad = (int)pad;
    pl.row_tile = GC_BM;
    pl.gy = C / GC_SPAN;
    if (op == GC_FWD) {
        s.Hs = (int)H; s.Ws = (int)W; s.Ho = (int)P; s.Wo = (int)Q;
        s.sstride = (int)stride; s.spad = (int)pad;
        pl.name = "fwd" + kw;
    } else {
        s.Hs = (int)P; s.Ws = (int)Q; s.Ho = (int)H; s.Wo = (int)W;
        s.sstride = 1;
        if (stride == 1) {
            s.spad = 2 - (int)pad;
            pl.name = "dgrad_s1" + kw;
        } else {
            s.spad = 0;
            pl.cls = true;
            pl.gz = 4;
            pl.name = "dgrad_s2cls" + kw;
        }
    }
    s.M = (int)(N * s.Ho * s.Wo);
    const long rows = pl.cls ? N * ((H + 1) / 2) * ((W + 1) / 2) : (long)s.M;
    pl.gx = ceil_div_i(rows, GC_BM);
    return pl;
}

std::tuple<std::string, long, long, long, long, long> gconv2d_plan(
        std::string op, long N, long C, long H, long W, long groups,
        long stride, long pad) {
    GcOp o;
    if (op == "fwd") o = GC_FWD;
    else if (op == "dgrad") o = GC_DGRAD;
    else if (op == "wgrad") o = GC_WGRAD;
    else TORCH_CHECK(false, "gconv2d_plan: op must be 'fwd', 'dgrad' or "
                     "'wgrad'; got '", op, "'");
    GcPlan pl = gc_plan(o, N, C, H, W, groups, stride, pad);
    return {pl.name, pl.row_tile, pl.gx, pl.gy, pl.gz, pl.split};
}

static void gc_check_act(const at::Tensor& t, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                t.dim() == 4, "gconv2d: ", what, " must be bf16 [N,C,H,W]");
    TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast),
                "gconv2d: ", what, " must be channels_last");
}

static void gc_check_image(const at::Tensor& img, long C) {
    TORCH_CHECK(img.is_cuda() && img.scalar_type() == at::kBFloat16 &&
                img.is_contiguous() && img.dim() == 4 &&
                img.size(0) == C / GC_SPAN && img.size(1) == 9 &&
                img.size(2) == GC_SPAN && img.size(3) == GC_SPAN,
                "gconv2d: the weight image must be the bf16 [C/64, 9, 64, 64] "
                "of gconv2d_pack");
}

static at::Tensor gc_empty_nhwc(const at::Tensor& like, long n, long c, long h,
                                long w) {
    return at::empty({n, c, h, w}, like.options().memory_format(
        at::MemoryFormat::ChannelsLast));
}

// w: the contiguous fp32 master [C, Cg, 3, 3] -> (forward image, dgrad image)
std::tuple<at::Tensor, at::Tensor> gconv2d_pack(at::Tensor w) {
    TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.dim() == 4 &&
                w.is_contiguous() && w.size(2) == 3 && w.size(3) == 3,
                "gconv2d_pack: w must be the contiguous fp32 [C,Cg,3,3]");
    const long C = w.size(0), Cg = w.size(1);
    TORCH_CHECK(Cg >= 1 && C % Cg == 0, "gconv2d_pack: bad weight shape");
    gc_check_scope(C, C / Cg, 1, 0);
    auto opt = w.options().dtype(at::kBFloat16);
    auto fwd = at::empty({C / GC_SPAN, 9, GC_SPAN, GC_SPAN}, opt);
    auto dgr = at::empty_like(fwd);
    const long total = C * 9 * GC_SPAN;
    hipLaunchKernelGGL(k_pack_gconv_weight, dim3(ceil_div_i(total, 256)),
                       dim3(256), 0, at::hip::getCurrentHIPStream().stream(),
                       w.data_ptr<float>(), (int)C, (int)Cg,
                       reinterpret_cast<unsigned short*>(fwd.data_ptr()),
                       reinterpret_cast<unsigned short*>(dgr.data_ptr()));
    HIP_CHECK_LAST();
    return {fwd, dgr};
}

template <int KW>
static void gc_launch(const GcPlan& pl, bool hb, bool stats,
                      const at::Tensor& src, const at::Tensor& img,
                      const float* bias, at::Tensor& out, float* slab) {
    auto kern = pl.cls ? k_gconv_fwd<KW, false, false, true>
        : stats ? (hb ? k_gconv_fwd<KW, true, true, false>
                      : k_gconv_fwd<KW, false, true, false>)
                : (hb ? k_gconv_fwd<KW, true, false, false>
                      : k_gconv_fwd<KW, false, false, false>);
    hipLaunchKernelGGL(kern, dim3(pl.gx, pl.gy, pl.gz), dim3(256), 0,
                       at::hip::getCurrentHIPStream().stream(),
                       reinterpret_cast<const bf16*>(src.data_ptr()),
                       reinterpret_cast<const bf16*>(img.data_ptr()), bias,
                       reinterpret_cast<bf16*>(out.data_ptr()), slab, pl.s);
    HIP_CHECK_LAST();
}

static void gc_dispatch(const GcPlan& pl, bool hb, bool stats,
                        const at::Tensor& src, const at::Tensor& img,
                        const float* bias, at::Tensor& out, float* slab) {
    if (pl.kw == 16) gc_launch<16>(pl, hb, stats, src, img, bias, out, slab);
    else if (pl.kw == 32)
        gc_launch<32>(pl, hb, stats, src, img, bias, out, slab);
    else gc_launch<64>(pl, hb, stats, src, img, bias, out, slab);
}

// x: bf16 [N,C,H,W] channels_last; wimg: the forward image.  Returns
// (y, slab); slab is the [2][C][row tiles] BN partial slab with want_stats,
// else undefined.
std::tuple<at::Tensor, at::Tensor> gconv2d_fwd(
        at::Tensor x, at::Tensor wimg, c10::optional<at::Tensor> bias,
        long groups, long stride, long pad, bool want_stats) {
    gc_check_act(x, "x");
    GcPlan pl = gc_plan(GC_FWD, x.size(0), x.size(1), x.size(2), x.size(3),
                        groups, stride, pad);
    gc_check_image(wimg, x.size(1));
    if (bias.has_value())
        TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == at::kFloat &&
                    bias->is_contiguous() && bias->numel() == x.size(1),
                    "gconv2d_fwd: bias must be fp32 [C]");
    auto y = gc_empty_nhwc(x, pl.s.N, pl.s.C, pl.s.Ho, pl.s.Wo);
    at::Tensor slab;
    if (want_stats)
        slab = at::empty({2, (long)pl.s.C, pl.gx},
                         x.options().dtype(at::kFloat));
    gc_dispatch(pl, bias.has_value(), want_stats, x, wimg,
                bias.has_value() ? bias->data_ptr<float>() : nullptr, y,
                want_stats ? slab.data_ptr<float>() : nullptr);
    return {y, slab};
}

// dy: bf16 [N,C,P,Q] channels_last of the conv over an [N,C,H,W] input;
// wimg_t: the dgrad image.  Every dx element is written by the kernel.
at::Tensor gconv2d_dgrad(at::Tensor dy, at::Tensor wimg_t, long H, long W,
                         long groups, long stride, long pad) {
    gc_check_act(dy, "dy");
    TORCH_CHECK(H >= 1 && W >= 1, "gconv2d_dgrad: bad H / W");
    GcPlan pl = gc_plan(GC_DGRAD, dy.size(0), dy.size(1), H, W, groups,
                        stride, pad);
    gc_check_image(wimg_t, dy.size(1));
    TORCH_CHECK(dy.size(2) == pl.s.Hs && dy.size(3) == pl.s.Ws,
                "gconv2d_dgrad: dy is not the output of this conv over "
                "[H, W] = [", H, ", ", W, "]");
    auto dx = gc_empty_nhwc(dy, pl.s.N, pl.s.C, H, W);
    gc_dispatch(pl, false, false, dy, wimg_t, nullptr, dx, nullptr);
    return dx;
}

// Returns dw fp32 [C, Cg, 3, 3].
at::Tensor gconv2d_wgrad(at::Tensor dy, at::Tensor x, long groups, long stride,
                         long pad) {
    gc_check_act(dy, "dy");
    gc_check_act(x, "x");
    GcPlan pl = gc_plan(GC_WGRAD, x.size(0), x.size(1), x.size(2), x.size(3),
                        groups, stride, pad);
    const GwShape& g = pl.w;
    TORCH_CHECK(dy.size(0) == x.size(0) && dy.size(1) == x.size(1) &&
                dy.size(2) == g.P && dy.size(3) == g.Q,
                "gconv2d_wgrad: dy is not the output of this conv over x");
    const long C = g.C, Cg = g.Cg, total = C * Cg * 9;
    auto fopt = x.options().dtype(at::kFloat);
    auto slab = at::empty({(long)pl.split, C, Cg, 9}, fopt);
    auto dw = at::empty({C, Cg, 3, 3}, fopt);
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto kern = pl.kw == 16 ? k_gconv_wgrad<16>
              : pl.kw == 32 ? k_gconv_wgrad<32> : k_gconv_wgrad<64>;
    hipLaunchKernelGGL(kern, dim3(pl.gx, pl.gy), dim3(256), 0, stream,
                       reinterpret_cast<const bf16*>(dy.data_ptr()),
                       reinterpret_cast<const bf16*>(x.data_ptr()),
                       slab.data_ptr<float>(), g);
    HIP_CHECK_LAST();
    const int cgx = ceil_div_i(total, 256);
    const float* src = slab.data_ptr<float>();
    int S = pl.split;
    at::Tensor slab2;
    if (S > GC_COMBINE_DIRECT) {
        const int nch = ceil_div_i(S, GC_COMBINE_CH);
        slab2 = at::empty({(long)nch, total}, fopt);
        hipLaunchKernelGGL(k_gconv_wgrad_combine, dim3(cgx, nch), dim3(256),
                           0, stream, src, S, GC_COMBINE_CH, total,
                           slab2.data_ptr<float>());
        HIP_CHECK_LAST();
        src = slab2.data_ptr<float>();
        S = nch;
    }
    hipLaunchKernelGGL(k_gconv_wgrad_combine, dim3(cgx, 1), dim3(256), 0,
                       stream, src, S, S, total, dw.data_ptr<float>());
    HIP_CHECK_LAST();
    return dw;
}
