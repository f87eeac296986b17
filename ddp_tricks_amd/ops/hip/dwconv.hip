// dwconv.hip — depthwise 3x3 convolution (groups == C_in == C_out), direct
// VALU kernels for gfx950.
//
// A depthwise conv has nine MACs per output element and no contraction over
// channels: nothing for the MFMA to contract, so forward, dgrad and wgrad are
// direct kernels in the style of k_conv_c1_r3_fwd (conv.hip).  Scope: 3x3,
// dilation 1, one stride (1 or 2) and one padding (0 or 1) for both dims,
// C % 8 == 0, bf16 channels_last activations, the fp32 master weight
// [C,1,3,3] read directly and rounded to bf16 with f2us (no pack launch, no
// cached weight image).
//
// Data movement, all kernels:
//   * A lane owns one 8-channel chunk (16 B) of one column.  The block's 256
//     lanes lie flat over (column, chunk): tid = col * slw + ck, so a wave's
//     loads and stores of one row are contiguous (1 KiB at C >= 512, 16
//     pixels at C = 32).  slw = min(C/8, 64) chunks; wider C puts further
//     channel slices on gridDim.y, so a lane's chunk — and its 72 weights —
//     is fixed for the block's life.  cb = 256 / slw columns per block; lanes
//     past cb * slw, past the last column or past C idle (lane_on).
//   * A work unit is (image, strip of tr rows, tile of cb columns); block b
//     takes units b, b + gridDim.x, ...  The lane walks down the strip with
//     the 3x3 input window in registers as fp32: each loaded chunk is
//     converted once, rows rotate through three register slots (the walk is
//     unrolled by three so the slot is a compile-time index), stride 1 loads
//     3 new chunks per output and stride 2 loads 6, and the next rows' loads
//     are issued before the current row's FMAs.
//   * Horizontal neighbours are other lanes of the same wave reading the
//     same lines: that reuse is left to the vector L1, activations do not
//     pass through LDS.
//   * Padding is a predicated load that yields zeros; the offset is formed
//     only under the predicate.
// Reductions (BN statistics, dw, db) are fixed-order: per-lane chains, a block
// join through LDS in index order (dw_block_join8), per-block slab slots and
// an in-order combine.  No fp atomics; every grid is a function of the shape
// alone (dw_plan, the one place that decides).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <algorithm>
#include <climits>
#include <string>
#include <tuple>
#include "common.h"

typedef short bf16x8_t __attribute__((ext_vector_type(8)));

// fp32 -> bf16 RNE on the hardware convert, as in conv.hip
DEV_INLINE short dw_f2bf_bits(float f) {
    return __builtin_bit_cast(short, (__bf16)f);
}

constexpr int DW_THREADS = 256;
constexpr int DW_MAX_SLW = 64;            // chunks per channel slice
constexpr int DW_TR_MAX = 16;             // rows per strip, automatic plan
constexpr int DW_MAX_BLOCKS = 1536;       // fwd / dgrad grid.x cap
constexpr int DW_WGRAD_MAX_BLOCKS = 512;  // wgrad grid.x cap (slab depth)
constexpr int DW_WGRAD_ROWS = 32;         // least row steps per wgrad block
constexpr int DW_COMBINE_CH = 32;         // stage-1 combine depth
constexpr int DW_COMBINE_DIRECT = 64;     // deeper slabs combine in two stages

struct DwShape {
    int N, C;
    int Hi, Wi;         // the tensor the window slides over
    int Ho, Wo;         // the tensor written (fwd, dgrad) / dy (wgrad)
    int rows, cols;     // walk extents: Ho, Wo except for dgrad_s2 (2x2 cells)
    int pad;            // 0..2 (stride-1 dgrad runs fwd with 2 - pad)
    int slw, cb, tr, nstrips, nct, units;
};

DEV_INLINE bf16x8_t dw_load(const bf16* base, bool ok, int row, int rowlen,
                            int colidx, int C) {
    bf16x8_t v = {};
    if (ok)
        v = *reinterpret_cast<const bf16x8_t*>(
            base + ((long)row * rowlen + colidx) * C);
    return v;
}

// Sums v[j] over the block's cb columns for every (chunk, j) of the slice, in
// index order, and hands channel c (0 .. slw*8) its total through emit(c, t)
// exactly once.  Two steps so that a narrow slice does not leave one thread
// adding 256 values: `parts` threads per channel add cpp consecutive columns
// each, then one thread adds the parts.  A value passes cpp + parts additions.
template <class F>
DEV_INLINE void dw_block_join8(const float (&v)[8], float (*red)[DW_THREADS + 8],
                               float* part, int slw, int cb, F&& emit) {
    const int tid = threadIdx.x;
    const int nch = slw * 8;
    const int parts = min(cb, max(1, DW_THREADS / nch));
    const int cpp = (cb + parts - 1) / parts;
    __syncthreads();                    // the previous join's readers
    #pragma unroll
    for (int j = 0; j < 8; ++j) red[j][tid] = v[j];
    __syncthreads();
    for (int idx = tid; idx < nch * parts; idx += DW_THREADS) {
        const int pt = idx / nch, c = idx - pt * nch;
        const int ck = c >> 3, j = c & 7;
        const int ce = min(cb, (pt + 1) * cpp);
        float t = 0.f;
        for (int col = pt * cpp; col < ce; ++col) t += red[j][col * slw + ck];
        part[idx] = t;
    }
    __syncthreads();
    for (int c = tid; c < nch; c += DW_THREADS) {
        float t = 0.f;
        for (int pt = 0; pt < parts; ++pt) t += part[pt * nch + c];
        emit(c, t);
    }
}

// ------------------------------------------------------------------ forward ---
// v = fmaf chain over the taps in (r, s) order from 0, + bias; y = bf16 RNE.
// FLIP reads tap 8 - k: the stride-1 dgrad is this kernel over dy with FLIP
// and pad' = 2 - pad.  STATS: per-lane fp32 sum / sum of squares of the
// pre-rounding v, joined per block into slab[2][C][gridDim.x] (the layout of
// conv2d_fwd_stats); every block writes its slot, idle lanes add zeros.
//
// Registers: window 72 + weights 72 + prefetch 12 (24 at stride 2) +
// statistics 16: 173 - 210 VGPRs over the instantiations, 2 waves/SIMD, no
// scratch.  NOTE: a 3-waves/SIMD bound (__launch_bounds__(256, 3), 168
// VGPRs) was tried and spills in every instantiation (5 - 81 VGPRs, 24 - 320
// B of scratch per lane; wgrad 38 - 146 VGPRs), so the bound stays at the
// block size.  What 2 waves/SIMD reach is in docs/KERNELS.md ("Depthwise
// conv"); packing the two older window rows as bf16 is the untried way down.
template <int STRIDE, bool FLIP, bool BIAS, bool STATS>
__global__ __launch_bounds__(DW_THREADS) NO_PK_F32
void k_dwconv3_fwd(const bf16* __restrict__ x, const float* __restrict__ w,
                   const float* __restrict__ bias, bf16* __restrict__ y,
                   float* __restrict__ slab, DwShape d) {
    const int tid = threadIdx.x;
    const int col = tid / d.slw, ck = tid - col * d.slw;
    const int chunk = blockIdx.y * d.slw + ck;
    const bool lane_on = col < d.cb && chunk * 8 < d.C;
    const int c0 = lane_on ? chunk * 8 : 0;

    float wr[9][8], bv[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
        #pragma unroll
        for (int k = 0; k < 9; ++k)
            wr[k][j] = us2f(f2us(w[(c0 + j) * 9 + (FLIP ? 8 - k : k)]));
        bv[j] = BIAS ? bias[c0 + j] : 0.f;
    }
    float sum[8] = {}, sq[8] = {};

    for (int u = blockIdx.x; u < d.units; u += gridDim.x) {
        const int t1 = u / d.nct, ct = u - t1 * d.nct;
        const int n = t1 / d.nstrips, st = t1 - n * d.nstrips;
        const int p0 = st * d.tr;
        const int nrows = min(d.tr, d.rows - p0);
        const int q = ct * d.cb + col;
        const bool on = lane_on && q < d.cols;
        const int iw0 = q * STRIDE - d.pad;
        const int ih0 = p0 * STRIDE - d.pad;
        bool cok[3];
        #pragma unroll
        for (int s = 0; s < 3; ++s)
            cok[s] = on && iw0 + s >= 0 && iw0 + s < d.Wi;
        const bf16* xn = x + (long)n * d.Hi * d.Wi * d.C + c0;
        bf16* yn = y + (long)n * d.Ho * d.Wo * d.C + c0;

        float win[3][3][8];
        #pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int ih = ih0 + r;
            const bool rok = ih >= 0 && ih < d.Hi;
            #pragma unroll
            for (int s = 0; s < 3; ++s) {
                bf16x8_t raw = dw_load(xn, rok && cok[s], ih, d.Wi, iw0 + s,
                                       d.C);
                #pragma unroll
                for (int j = 0; j < 8; ++j)
                    win[r][s][j] = us2f((unsigned short)raw[j]);
            }
        }
        for (int tb = 0; tb < nrows; tb += 3) {
            #pragma unroll
            for (int tt = 0; tt < 3; ++tt) {
                const int t = tb + tt;
                if (t < nrows) {
                    // the rows the next output adds, in flight over the FMAs
                    bf16x8_t nxt[STRIDE][3];
                    const bool more = t + 1 < nrows;
                    #pragma unroll
                    for (int i = 0; i < STRIDE; ++i) {
                        const int ih = ih0 + STRIDE * t + 3 + i;
                        const bool rok = more && ih >= 0 && ih < d.Hi;
                        #pragma unroll
                        for (int s = 0; s < 3; ++s)
                            nxt[i][s] = dw_load(xn, rok && cok[s], ih, d.Wi,
                                                iw0 + s, d.C);
                    }
                    bf16x8_t o;
                    #pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float v = 0.f;
                        #pragma unroll
                        for (int r = 0; r < 3; ++r)
                            #pragma unroll
                            for (int s = 0; s < 3; ++s)
                                v = fmaf(win[(STRIDE * tt + r) % 3][s][j],
                                         wr[r * 3 + s][j], v);
                        if (BIAS) v += bv[j];
                        if (STATS) {
                            const float vs = on ? v : 0.f;
                            sum[j] += vs;
                            sq[j] = fmaf(vs, vs, sq[j]);
                        }
                        o[j] = dw_f2bf_bits(v);
                    }
                    if (on)
                        *reinterpret_cast<bf16x8_t*>(
                            yn + ((long)(p0 + t) * d.Wo + q) * d.C) = o;
                    #pragma unroll
                    for (int i = 0; i < STRIDE; ++i)
                        #pragma unroll
                        for (int s = 0; s < 3; ++s)
                            #pragma unroll
                            for (int j = 0; j < 8; ++j)
                                win[(STRIDE * tt + i) % 3][s][j] =
                                    us2f((unsigned short)nxt[i][s][j]);
                }
            }
        }
    }
    if constexpr (STATS) {
        __shared__ float red[8][DW_THREADS + 8];
        __shared__ float part[DW_MAX_SLW * 8];
        const int cbase = blockIdx.y * d.slw * 8;
        dw_block_join8(sum, red, part, d.slw, d.cb, [&](int c, float t) {
            if (cbase + c < d.C)
                slab[(long)(cbase + c) * gridDim.x + blockIdx.x] = t;
        });
        dw_block_join8(sq, red, part, d.slw, d.cb, [&](int c, float t) {
            if (cbase + c < d.C)
                slab[((long)d.C + cbase + c) * gridDim.x + blockIdx.x] = t;
        });
    }
}

// ---------------------------------------------------------- dgrad, stride 2 ---
// dx[h][w] = sum over the taps (r, s) with h + pad - r and w + pad - s even
// of dy[(h + pad - r) / 2][(w + pad - s) / 2] * w[r][s].  In padded
// coordinates a = h + pad, b = w + pad the four pixels a in {2i, 2i + 1},
// b in {2j, 2j + 1} read only the 2x2 window dy[i-1 .. i][j-1 .. j]:
//   (even, even)  w00 dy[i][j] + w02 dy[i][j-1] + w20 dy[i-1][j] + w22 dy[i-1][j-1]
//   (even, odd)   w01 dy[i][j] + w21 dy[i-1][j]
//   (odd,  even)  w10 dy[i][j] + w12 dy[i][j-1]
//   (odd,  odd)   w11 dy[i][j]
// 4 + 2 + 2 + 1 = 9 MACs, no zero tap multiplied.  A lane owns cell (i, j)
// of one chunk and walks down i keeping the window's two rows in registers
// (one new row, 2 chunks, per cell).  The cells i = 0 .. (H-1+pad)/2,
// j = 0 .. (W-1+pad)/2 tile dx exactly, so every dx pixel is written once —
// trailing rows / columns no output reads get their zeros here, no pre-pass.
__global__ __launch_bounds__(DW_THREADS) NO_PK_F32
void k_dwconv3_dgrad_s2(const bf16* __restrict__ dy,
                        const float* __restrict__ w, bf16* __restrict__ dx,
                        DwShape d) {
    const int tid = threadIdx.x;
    const int col = tid / d.slw, ck = tid - col * d.slw;
    const int chunk = blockIdx.y * d.slw + ck;
    const bool lane_on = col < d.cb && chunk * 8 < d.C;
    const int c0 = lane_on ? chunk * 8 : 0;

    float wr[9][8];
    #pragma unroll
    for (int j = 0; j < 8; ++j)
        #pragma unroll
        for (int k = 0; k < 9; ++k)
            wr[k][j] = us2f(f2us(w[(c0 + j) * 9 + k]));

    for (int u = blockIdx.x; u < d.units; u += gridDim.x) {
        const int t1 = u / d.nct, ct = u - t1 * d.nct;
        const int n = t1 / d.nstrips, st = t1 - n * d.nstrips;
        const int i0 = st * d.tr;
        const int nrows = min(d.tr, d.rows - i0);
        const int jc = ct * d.cb + col;
        const bool on = lane_on && jc < d.cols;
        // window columns jc - 1 (index 0) and jc (index 1) of dy
        const bool cok[2] = {on && jc - 1 >= 0 && jc - 1 < d.Wi,
                             on && jc < d.Wi};
        const int wx = 2 * jc - d.pad;          // dx columns wx, wx + 1
        const bool wok[2] = {on && wx >= 0 && wx < d.Wo,
                             on && wx + 1 >= 0 && wx + 1 < d.Wo};
        const bf16* dyn = dy + (long)n * d.Hi * d.Wi * d.C + c0;
        bf16* dxn = dx + (long)n * d.Ho * d.Wo * d.C + c0;

        float top[2][8], bot[2][8];
        bf16x8_t nxt[2];
        {
            const int ih = i0 - 1;
            const bool rok = ih >= 0 && ih < d.Hi;
            #pragma unroll
            for (int s = 0; s < 2; ++s) {
                bf16x8_t raw = dw_load(dyn, rok && cok[s], ih, d.Wi,
                                       jc - 1 + s, d.C);
                #pragma unroll
                for (int j = 0; j < 8; ++j)
                    top[s][j] = us2f((unsigned short)raw[j]);
            }
            const bool rok1 = i0 < d.Hi;
            #pragma unroll
            for (int s = 0; s < 2; ++s)
                nxt[s] = dw_load(dyn, rok1 && cok[s], i0, d.Wi, jc - 1 + s,
                                 d.C);
        }
        for (int t = 0; t < nrows; ++t) {
            const int i = i0 + t;
            #pragma unroll
            for (int s = 0; s < 2; ++s)
                #pragma unroll
                for (int j = 0; j < 8; ++j)
                    bot[s][j] = us2f((unsigned short)nxt[s][j]);
            {   // row i + 1, in flight over the FMAs
                const bool rok = t + 1 < nrows && i + 1 < d.Hi;
                #pragma unroll
                for (int s = 0; s < 2; ++s)
                    nxt[s] = dw_load(dyn, rok && cok[s], i + 1, d.Wi,
                                     jc - 1 + s, d.C);
            }
            bf16x8_t o[2][2];
            #pragma unroll
            for (int j = 0; j < 8; ++j) {
                float ee = fmaf(bot[1][j], wr[0][j], 0.f);
                ee = fmaf(bot[0][j], wr[2][j], ee);
                ee = fmaf(top[1][j], wr[6][j], ee);
                ee = fmaf(top[0][j], wr[8][j], ee);
                float eo = fmaf(bot[1][j], wr[1][j], 0.f);
                eo = fmaf(top[1][j], wr[7][j], eo);
                float oe = fmaf(bot[1][j], wr[3][j], 0.f);
                oe = fmaf(bot[0][j], wr[5][j], oe);
                const float oo = bot[1][j] * wr[4][j];
                o[0][0][j] = dw_f2bf_bits(ee);
                o[0][1][j] = dw_f2bf_bits(eo);
                o[1][0][j] = dw_f2bf_bits(oe);
                o[1][1][j] = dw_f2bf_bits(oo);
            }
            #pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int h = 2 * i + a - d.pad;
                const bool hok = h >= 0 && h < d.Ho;
                #pragma unroll
                for (int b = 0; b < 2; ++b)
                    if (hok && wok[b])
                        *reinterpret_cast<bf16x8_t*>(
                            dxn + ((long)h * d.Wo + wx + b) * d.C) = o[a][b];
            }
            #pragma unroll
            for (int s = 0; s < 2; ++s)
                #pragma unroll
                for (int j = 0; j < 8; ++j) top[s][j] = bot[s][j];
        }
    }
}

// -------------------------------------------------------------------- wgrad ---
// dw[c][r][s] = sum over (n, p, q) of dy[n][p][q][c] * x[n][p*S-pad+r][q*S-pad+s][c].
// The forward kernel's walk and window plus one dy chunk per output pixel
// (dy is read once; DB adds it into 8 more accumulators).  A lane keeps its
// 72 (+8) fp32 sums over all of the block's units; at the end the lanes that
// share a chunk are joined through LDS, tap by tap, into
// slab[block][9 (+1)][C].  k_dwconv3_wgrad_combine sums the blocks in order.
template <int STRIDE, bool DB>
__global__ __launch_bounds__(DW_THREADS) NO_PK_F32
void k_dwconv3_wgrad(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                     float* __restrict__ slab, DwShape d) {
    const int tid = threadIdx.x;
    const int col = tid / d.slw, ck = tid - col * d.slw;
    const int chunk = blockIdx.y * d.slw + ck;
    const bool lane_on = col < d.cb && chunk * 8 < d.C;
    const int c0 = lane_on ? chunk * 8 : 0;

    float acc[9][8] = {}, dba[8] = {};

    for (int u = blockIdx.x; u < d.units; u += gridDim.x) {
        const int t1 = u / d.nct, ct = u - t1 * d.nct;
        const int n = t1 / d.nstrips, st = t1 - n * d.nstrips;
        const int p0 = st * d.tr;
        const int nrows = min(d.tr, d.rows - p0);
        const int q = ct * d.cb + col;
        const bool on = lane_on && q < d.cols;
        const int iw0 = q * STRIDE - d.pad;
        const int ih0 = p0 * STRIDE - d.pad;
        bool cok[3];
        #pragma unroll
        for (int s = 0; s < 3; ++s)
            cok[s] = on && iw0 + s >= 0 && iw0 + s < d.Wi;
        const bf16* xn = x + (long)n * d.Hi * d.Wi * d.C + c0;
        const bf16* dyn = dy + (long)n * d.Ho * d.Wo * d.C + c0;

        float win[3][3][8];
        #pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int ih = ih0 + r;
            const bool rok = ih >= 0 && ih < d.Hi;
            #pragma unroll
            for (int s = 0; s < 3; ++s) {
                bf16x8_t raw = dw_load(xn, rok && cok[s], ih, d.Wi, iw0 + s,
                                       d.C);
                #pragma unroll
                for (int j = 0; j < 8; ++j)
                    win[r][s][j] = us2f((unsigned short)raw[j]);
            }
        }
        bf16x8_t gn = dw_load(dyn, on, p0, d.Wo, q, d.C);
        for (int tb = 0; tb < nrows; tb += 3) {
            #pragma unroll
            for (int tt = 0; tt < 3; ++tt) {
                const int t = tb + tt;
                if (t < nrows) {
                    float g[8];
                    #pragma unroll
                    for (int j = 0; j < 8; ++j)
                        g[j] = us2f((unsigned short)gn[j]);
                    bf16x8_t nxt[STRIDE][3];
                    const bool more = t + 1 < nrows;
                    #pragma unroll
                    for (int i = 0; i < STRIDE; ++i) {
                        const int ih = ih0 + STRIDE * t + 3 + i;
                        const bool rok = more && ih >= 0 && ih < d.Hi;
                        #pragma unroll
                        for (int s = 0; s < 3; ++s)
                            nxt[i][s] = dw_load(xn, rok && cok[s], ih, d.Wi,
                                                iw0 + s, d.C);
                    }
                    gn = dw_load(dyn, on && more, p0 + t + 1, d.Wo, q, d.C);
                    #pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        #pragma unroll
                        for (int r = 0; r < 3; ++r)
                            #pragma unroll
                            for (int s = 0; s < 3; ++s)
                                acc[r * 3 + s][j] =
                                    fmaf(g[j], win[(STRIDE * tt + r) % 3][s][j],
                                         acc[r * 3 + s][j]);
                        if (DB) dba[j] += g[j];
                    }
                    #pragma unroll
                    for (int i = 0; i < STRIDE; ++i)
                        #pragma unroll
                        for (int s = 0; s < 3; ++s)
                            #pragma unroll
                            for (int j = 0; j < 8; ++j)
                                win[(STRIDE * tt + i) % 3][s][j] =
                                    us2f((unsigned short)nxt[i][s][j]);
                }
            }
        }
    }
    __shared__ float red[8][DW_THREADS + 8];
    __shared__ float part[DW_MAX_SLW * 8];
    const int cbase = blockIdx.y * d.slw * 8;
    constexpr int KK = DB ? 10 : 9;
    float* mine = slab + (long)blockIdx.x * KK * d.C;
    #pragma unroll
    for (int k = 0; k < 9; ++k)
        dw_block_join8(acc[k], red, part, d.slw, d.cb, [&](int c, float t) {
            if (cbase + c < d.C) mine[(long)k * d.C + cbase + c] = t;
        });
    if constexpr (DB)
        dw_block_join8(dba, red, part, d.slw, d.cb, [&](int c, float t) {
            if (cbase + c < d.C) mine[(long)9 * d.C + cbase + c] = t;
        });
}

// slab[S][total] summed over s in fixed order, total = (9 or 10) * C and
// i = k * C + c.  FINAL writes dw[c][k] (torch [C,1,3,3]) and db[c] from the
// whole depth; otherwise block row blockIdx.y sums slices [y*CH, y*CH + CH)
// into out[y][i] (stage 1 of a deep slab, as k_wgrad_combine_stage: one
// thread chewing hundreds of strided dependent loads is latency-bound).
// Two chains, even / odd slices, keep two loads in flight; the order is fixed.
template <bool FINAL>
__global__ void k_dwconv3_wgrad_combine(const float* __restrict__ slab, int S,
                                        int CH, long total, int C,
                                        float* __restrict__ out,
                                        float* __restrict__ db) {
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
    const float v = v0 + v1;
    if (!FINAL) {
        out[(long)blockIdx.y * total + i] = v;
    } else {
        const int k = (int)(i / C), c = (int)(i - (long)k * C);
        if (k < 9) out[(long)c * 9 + k] = v;
        else db[c] = v;
    }
}

// -------------------------------------------------------------------- hosts ---

enum DwOp { DW_FWD = 0, DW_DGRAD = 1, DW_WGRAD = 2 };

struct DwPlan {
    DwShape d;
    int gx, gy;
};

// The one place that decides slice width, strip height and grid; pure host
// arithmetic on the shape.  (N, C, H, W) is always the conv's input x.
// tr: -1 automatic, else the strip height (benchmarks and tests).
//   * slw = min(C/8, 64), gy = ceil(C/8 / slw), cb = 256 / slw.
//   * tr: the rows split into the fewest strips of at most DW_TR_MAX rows,
//     evenly (P = 56 -> 4 x 14, not 3 x 16 + 8).  Taller strips re-read fewer
//     halo rows (2 of tr + 2 at stride 1) but leave fewer units.  Measured
//     forward at B = 256 (profiles/bench_kernels_dwconv.log), us at tr 4 / 8 /
//     plan / 32: C32 H112 s1 156.6 / 147.8 / 141.9 / 155.3; C128 H56 s1
//     155.8 / 146.4 / 142.6 / 153.5; C64 H112 s2 112.1 / 107.5 / 108.1 /
//     115.7; C512 H14 s1 39.4 / 34.9 / 28.6 / 28.5.  Where P = 28 the plan's
//     2 x 14 loses to one strip (C256 s1 51.6 vs 47.5, C128 H56 s2 42.5 vs
//     40.8).  At C256 the 2048 units on 1536 blocks leave a second,
//     one-third-full round; the cause at C128 (1024 units) is not known.
//     Not acted on here: "one strip up to 32 rows" is the follow-up to
//     measure.
//   * gx: fwd / dgrad min(units, DW_MAX_BLOCKS); wgrad additionally at most
//     units * tr / DW_WGRAD_ROWS (a block's ten joins want some rows to
//     amortise over) and DW_WGRAD_MAX_BLOCKS (the slab's depth).
static DwPlan dw_plan(DwOp op, long N, long C, long H, long W, long stride,
                      long pad, long tr) {
    TORCH_CHECK(N >= 1 && C >= 8 && C % 8 == 0, "dwconv2d: C must be a "
                "positive multiple of 8; got N=", N, " C=", C);
    TORCH_CHECK((stride == 1 || stride == 2) && (pad == 0 || pad == 1),
                "dwconv2d: stride must be 1 or 2 and padding 0 or 1; got "
                "stride=", stride, " pad=", pad);
    TORCH_CHECK(H + 2 * pad >= 3 && W + 2 * pad >= 3,
                "dwconv2d: input smaller than the 3x3 window");
    TORCH_CHECK(tr == -1 || tr >= 1, "dwconv2d: tr must be -1 or positive");
    const long P = (H + 2 * pad - 3) / stride + 1;
    const long Q = (W + 2 * pad - 3) / stride + 1;
    TORCH_CHECK(H <= (1 << 24) && W <= (1 << 24) && C <= (1 << 24) &&
                N * H * W < INT_MAX, "dwconv2d: index range");
    DwShape d;
    d.N = (int)N; d.C = (int)C;
    d.pad = (int)pad;
    if (op == DW_DGRAD) {
        d.Hi = (int)P; d.Wi = (int)Q; d.Ho = (int)H; d.Wo = (int)W;
        if (stride == 1) {
            d.rows = d.Ho; d.cols = d.Wo;
            d.pad = 2 - (int)pad;
        } else {
            d.rows = (int)((H - 1 + pad) / 2 + 1);
            d.cols = (int)((W - 1 + pad) / 2 + 1);
        }
    } else {
        d.Hi = (int)H; d.Wi = (int)W; d.Ho = (int)P; d.Wo = (int)Q;
        d.rows = d.Ho; d.cols = d.Wo;
    }
    const int chunks = d.C / 8;
    d.slw = std::min(chunks, DW_MAX_SLW);
    d.cb = DW_THREADS / d.slw;
    d.tr = tr > 0 ? (int)std::min<long>(tr, d.rows)
                  : ceil_div_i(d.rows, ceil_div_i(d.rows, DW_TR_MAX));
    d.nstrips = ceil_div_i(d.rows, d.tr);
    d.nct = ceil_div_i(d.cols, d.cb);
    const long units = N * d.nstrips * d.nct;
    TORCH_CHECK(units < INT_MAX, "dwconv2d: too many work units");
    d.units = (int)units;
    DwPlan pl;
    pl.d = d;
    pl.gy = ceil_div_i(chunks, d.slw);
    long gx = std::min<long>(units, DW_MAX_BLOCKS);
    if (op == DW_WGRAD)
        gx = std::min<long>(units, std::max<long>(1, std::min<long>(
            DW_WGRAD_MAX_BLOCKS, units * d.tr / DW_WGRAD_ROWS)));
    pl.gx = (int)gx;
    return pl;
}

std::tuple<long, long, long, long> dwconv2d_plan(std::string op, long N,
                                                 long C, long H, long W,
                                                 long stride, long pad,
                                                 long tr) {
    DwOp o;
    if (op == "fwd") o = DW_FWD;
    else if (op == "dgrad") o = DW_DGRAD;
    else if (op == "wgrad") o = DW_WGRAD;
    else TORCH_CHECK(false, "dwconv2d_plan: op must be 'fwd', 'dgrad' or "
                     "'wgrad'; got '", op, "'");
    DwPlan pl = dw_plan(o, N, C, H, W, stride, pad, tr);
    return {pl.d.slw, pl.d.tr, pl.gx, pl.gy};
}

static void dw_check_act(const at::Tensor& t, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                t.dim() == 4, "dwconv2d: ", what, " must be bf16 [N,C,H,W]");
    TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast),
                "dwconv2d: ", what, " must be channels_last");
}

static void dw_check_weight(const at::Tensor& w, long C) {
    TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.dim() == 4 &&
                w.is_contiguous() && w.size(0) == C && w.size(1) == 1 &&
                w.size(2) == 3 && w.size(3) == 3,
                "dwconv2d: w must be the contiguous fp32 [C,1,3,3]");
}

static at::Tensor dw_empty_nhwc(const at::Tensor& like, long n, long c, long h,
                                long w) {
    return at::empty({n, c, h, w}, like.options().memory_format(
        at::MemoryFormat::ChannelsLast));
}

template <int STRIDE, bool FLIP>
static void dw_launch_fwd(const DwPlan& pl, bool hb, bool stats,
                          const at::Tensor& x, const at::Tensor& w,
                          const float* bias, at::Tensor& y, float* slab) {
    auto kern = stats
        ? (hb ? k_dwconv3_fwd<STRIDE, FLIP, true, true>
              : k_dwconv3_fwd<STRIDE, FLIP, false, true>)
        : (hb ? k_dwconv3_fwd<STRIDE, FLIP, true, false>
              : k_dwconv3_fwd<STRIDE, FLIP, false, false>);
    hipLaunchKernelGGL(kern, dim3(pl.gx, pl.gy), dim3(DW_THREADS), 0,
                       at::hip::getCurrentHIPStream().stream(),
                       reinterpret_cast<const bf16*>(x.data_ptr()),
                       w.data_ptr<float>(), bias,
                       reinterpret_cast<bf16*>(y.data_ptr()), slab, pl.d);
    HIP_CHECK_LAST();
}

// x: bf16 [N,C,H,W] channels_last; w: the fp32 master [C,1,3,3].  Returns
// (y, slab); slab is the [2][C][gx] BN partial slab with want_stats, else
// undefined.
std::tuple<at::Tensor, at::Tensor> dwconv2d_fwd(
        at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias,
        long stride, long pad, bool want_stats, long tr) {
    dw_check_act(x, "x");
    dw_check_weight(w, x.size(1));
    if (bias.has_value())
        TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == at::kFloat &&
                    bias->is_contiguous() && bias->numel() == x.size(1),
                    "dwconv2d_fwd: bias must be fp32 [C]");
    DwPlan pl = dw_plan(DW_FWD, x.size(0), x.size(1), x.size(2), x.size(3),
                        stride, pad, tr);
    auto y = dw_empty_nhwc(x, pl.d.N, pl.d.C, pl.d.Ho, pl.d.Wo);
    at::Tensor slab;
    if (want_stats)
        slab = at::empty({2, (long)pl.d.C, (long)pl.gx},
                         x.options().dtype(at::kFloat));
    const float* bp = bias.has_value() ? bias->data_ptr<float>() : nullptr;
    float* sp = want_stats ? slab.data_ptr<float>() : nullptr;
    if (stride == 1)
        dw_launch_fwd<1, false>(pl, bias.has_value(), want_stats, x, w, bp, y,
                                sp);
    else
        dw_launch_fwd<2, false>(pl, bias.has_value(), want_stats, x, w, bp, y,
                                sp);
    return {y, slab};
}

// dy: bf16 [N,C,P,Q] channels_last of the conv over an [N,C,H,W] input.
// Stride 1 is the forward kernel with flipped taps and pad 2 - pad; stride 2
// the 2x2-cell kernel.  Every dx element is written by the kernel.
at::Tensor dwconv2d_dgrad(at::Tensor dy, at::Tensor w, long H, long W,
                          long stride, long pad, long tr) {
    dw_check_act(dy, "dy");
    dw_check_weight(w, dy.size(1));
    TORCH_CHECK(H >= 1 && W >= 1, "dwconv2d_dgrad: bad H / W");
    DwPlan pl = dw_plan(DW_DGRAD, dy.size(0), dy.size(1), H, W, stride, pad,
                        tr);
    TORCH_CHECK(dy.size(2) == pl.d.Hi && dy.size(3) == pl.d.Wi,
                "dwconv2d_dgrad: dy is not the output of this conv over "
                "[H, W] = [", H, ", ", W, "]");
    auto dx = dw_empty_nhwc(dy, pl.d.N, pl.d.C, H, W);
    if (stride == 1) {
        dw_launch_fwd<1, true>(pl, false, false, dy, w, nullptr, dx, nullptr);
    } else {
        hipLaunchKernelGGL(k_dwconv3_dgrad_s2, dim3(pl.gx, pl.gy),
                           dim3(DW_THREADS), 0,
                           at::hip::getCurrentHIPStream().stream(),
                           reinterpret_cast<const bf16*>(dy.data_ptr()),
                           w.data_ptr<float>(),
                           reinterpret_cast<bf16*>(dx.data_ptr()), pl.d);
        HIP_CHECK_LAST();
    }
    return dx;
}

// Returns (dw fp32 [C,1,3,3], db fp32 [C]); db is undefined without want_db.
std::tuple<at::Tensor, at::Tensor> dwconv2d_wgrad(at::Tensor dy, at::Tensor x,
                                                  long stride, long pad,
                                                  bool want_db, long tr) {
    dw_check_act(dy, "dy");
    dw_check_act(x, "x");
    DwPlan pl = dw_plan(DW_WGRAD, x.size(0), x.size(1), x.size(2), x.size(3),
                        stride, pad, tr);
    TORCH_CHECK(dy.size(0) == x.size(0) && dy.size(1) == x.size(1) &&
                dy.size(2) == pl.d.Ho && dy.size(3) == pl.d.Wo,
                "dwconv2d_wgrad: dy is not the output of this conv over x");
    const long C = pl.d.C, KK = want_db ? 10 : 9, total = KK * C;
    auto fopt = x.options().dtype(at::kFloat);
    auto slab = at::empty({(long)pl.gx, KK, C}, fopt);
    auto dw = at::empty({C, 1, 3, 3}, fopt);
    at::Tensor db;
    if (want_db) db = at::empty({C}, fopt);
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto kern = stride == 1
        ? (want_db ? k_dwconv3_wgrad<1, true> : k_dwconv3_wgrad<1, false>)
        : (want_db ? k_dwconv3_wgrad<2, true> : k_dwconv3_wgrad<2, false>);
    hipLaunchKernelGGL(kern, dim3(pl.gx, pl.gy), dim3(DW_THREADS), 0, stream,
                       reinterpret_cast<const bf16*>(dy.data_ptr()),
                       reinterpret_cast<const bf16*>(x.data_ptr()),
                       slab.data_ptr<float>(), pl.d);
    HIP_CHECK_LAST();
    const int cgx = ceil_div_i(total, 256);
    const float* src = slab.data_ptr<float>();
    int S = pl.gx;
    at::Tensor slab2;
    if (S > DW_COMBINE_DIRECT) {
        const int nch = ceil_div_i(S, DW_COMBINE_CH);
        slab2 = at::empty({(long)nch, total}, fopt);
        hipLaunchKernelGGL(k_dwconv3_wgrad_combine<false>, dim3(cgx, nch),
                           dim3(256), 0, stream, src, S, DW_COMBINE_CH, total,
                           (int)C, slab2.data_ptr<float>(), (float*)nullptr);
        HIP_CHECK_LAST();
        src = slab2.data_ptr<float>();
        S = nch;
    }
    hipLaunchKernelGGL(k_dwconv3_wgrad_combine<true>, dim3(cgx, 1), dim3(256),
                       0, stream, src, S, S, total, (int)C,
                       dw.data_ptr<float>(),
                       want_db ? db.data_ptr<float>() : nullptr);
    HIP_CHECK_LAST();
    return {dw, db};
}
