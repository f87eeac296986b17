// dwconvk.hip — depthwise 5x5 and 7x7 convolution (groups == C_in == C_out),
// direct VALU kernels for gfx950 on an LDS tile.
//
// Scope: (K, stride) in {(5,1), (5,2), (7,1)}, dilation 1, one padding
// 0 .. K/2 for both dims, C % 8 == 0, bf16 channels_last activations, the
// fp32 master weight [C,1,K,K] read directly and rounded to bf16 with f2us
// (no pack launch, no cached weight image).  3x3 stays on dwconv.hip: that
// design keeps the KxK window and the K*K*8 weights of a lane's chunk in
// registers (72 + 72 at 3x3); at 5x5 that is 200 + 200, at 7x7 392 + 392.
//
// Forward / dgrad, column-tap-stationary on an LDS tile:
//   * A lane owns one 8-channel chunk (16 B) of one output column and a
//     vertical run of `to` output rows: TO x 8 fp32 accumulators, compile-time
//     indices only.  The 256 lanes lie flat over (column, chunk):
//     tid = col * slw + ck, slw = min(C/8, 16) chunks per channel slice
//     (further slices on gridDim.y), cb = 256 / slw columns.
//   * A work unit is (image, run of `to` rows, tile of cb columns); block b
//     takes units b, b + gridDim.x, ...  The block stages the unit's input
//     tile — (to-1)*S + K rows x (cb-1)*S + K columns x slw chunks of bf16 —
//     by __builtin_amdgcn_global_load_lds, 16 B per lane, no VGPR round trip.
//     The tile is entry-linear ((row * tcols + col) * slw + ck), so a wave's
//     64 lanes write 1 KiB in a row; an entry outside the image or past C
//     sources the zeroed 16 B buffer.  Padding is data: the compute loop has
//     no bounds test.
//   * For each kernel column s' (K passes) the lane holds that column's K x 8
//     weights as fp32 and walks down the tile rows j of its input column
//     q*S + s': one ds_read_b128 and one conversion per row, then fmaf into
//     the accumulator of every output row t with r = j - t*S in [0, K).  A
//     chunk is read and converted K times per unit instead of K*K times.
//   * The slice's weights are staged once per block into LDS as fp32,
//     transposed to [s'][r][chunk][8] (K*K*16*32 B: 12.5 KiB at 5x5, 24.5 KiB
//     at 7x7).  fp32 rather than bf16 bits because it fits: tile + weights is
//     72.5 / 79.5 / 74.5 KiB for K5s1 / K7s1 / K5s2, all <= 80 KiB, so two
//     blocks share a CU's 160 KiB, and the weight read needs no shifts.
//   * Each accumulator is a chain of K*K fmaf from 0 in (s', r) order, then
//     + bias, then bf16 RNE on the hardware convert.
// Wgrad puts the tap rows onto lanes (k_dwconvk_wgrad).  Reductions (BN
// statistics, dw, db) are fixed-order: per-lane chains, a block join through
// LDS in index order, per-block slab slots and an in-order combine.  No fp
// atomics; every grid is a function of the shape alone (dk_plan, the one
// place that decides).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <algorithm>
#include <climits>
#include <string>
#include <tuple>
#include "common.h"

typedef short dk_bf16x8 __attribute__((ext_vector_type(8)));

__device__ __align__(16) unsigned char dk_zero16[16];

constexpr int DK_THREADS = 256;
constexpr int DK_MAX_SLW = 16;            // chunks per channel slice
constexpr int DK_MAX_BLOCKS = 1024;       // fwd / dgrad grid.x cap
constexpr int DK_WGRAD_MAX_BLOCKS = 512;  // wgrad grid.x cap (slab depth)
constexpr int DK_WGRAD_UNITS = 4;         // least row groups per wgrad block
constexpr int DK_COMBINE_CH = 32;         // stage-1 combine depth
constexpr int DK_COMBINE_DIRECT = 64;     // deeper slabs combine in two stages
constexpr int DK_CELL_TO = 2;             // dgrad_s2: cells per run

// Output rows per run and the LDS tile of one (K, STRIDE) at slw = 16, where
// the tile is largest: rows * tcols * slw = rows * (256 S + (K - S) slw).
template <int K, int STRIDE>
struct DkTile {
    static constexpr int TO = STRIDE == 2 ? 2 : (K == 5 ? 8 : 4);
    static constexpr int TROWS = (TO - 1) * STRIDE + K;
    static constexpr int ENTRIES =
        (TROWS * (256 * STRIDE + (K - STRIDE) * DK_MAX_SLW) + 63) / 64 * 64;
};

struct DkShape {
    int N, C, chunks;
    int Hi, Wi;         // the tensor the tile is staged from
    int Ho, Wo;         // the tensor written (fwd, dgrad) / dy (wgrad)
    int rows, cols;     // walk extents: Ho, Wo except for dgrad_s2 (2x2 cells)
    int pad;            // 0 .. K-1 (stride-1 dgrad runs fwd with K-1-pad)
    int slw, cb, to, nruns, nct, units;
    int trows, tcols;   // tile extents
    FastDiv fslw;
};

DEV_INLINE short dk_f2bf_bits(float f) {
    return __builtin_bit_cast(short, (__bf16)f);
}

DEV_INLINE void dk_dma16(unsigned long src, bf16* lds_dst) {
    __builtin_amdgcn_global_load_lds(
        reinterpret_cast<const __attribute__((address_space(1)))
                         unsigned short*>(src),
        (__attribute__((address_space(3))) unsigned short*)lds_dst, 16, 0, 0);
}

// The block barrier, spelled out: the kernels are NO_PK_F32 and
// a function without that attribute (__syncthreads) is not inlined into one
// that has it, which made each barrier a call.  LAND first waits for this
// wave's in-flight global_load_lds, so the tile is whole behind the barrier.
template <bool LAND>
DEV_INLINE void dk_barrier() {
    if (LAND) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Stages tile rows [0, trows) x columns [0, tcols) x the slice's slw chunks
// of image `srcn` (already offset to the slice's first channel), tile origin
// (ih0, iw0).  Wave w takes entries [64 w + 256 i, + 64); a lane's entry
// advances by 256 <= tcols * slw per call, so its row steps by at most one:
// no division but the one by slw.  Entries past the tile's end land in the
// allocation's round-up to 64 entries.
DEV_INLINE void dk_stage(const bf16* srcn, int ih0, int iw0, const DkShape& d,
                         int nck, bf16* tile, unsigned long zaddr) {
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rowe = d.tcols * d.slw;
    const int ne = d.trows * rowe;
    int j = 0, rem = wid * 64 + lane;
    for (int e0 = wid * 64; e0 < ne; e0 += DK_THREADS) {
        const int cidx = (int)fd_div((unsigned)rem, d.fslw);
        const int ck = rem - cidx * d.slw;
        const int ih = ih0 + j, iw = iw0 + cidx;
        const bool ok = j < d.trows && (unsigned)ih < (unsigned)d.Hi &&
                        (unsigned)iw < (unsigned)d.Wi && ck < nck;
        const unsigned long a = reinterpret_cast<unsigned long>(srcn) +
            (unsigned long)((((long)ih * d.Wi + iw) * d.C + ck * 8) *
                            (long)sizeof(bf16));
        dk_dma16(ok ? a : zaddr, tile + (long)e0 * 8);
        rem += DK_THREADS;
        if (rem >= rowe) { rem -= rowe; ++j; }
    }
}

// The slice's weights into LDS as fp32, [s'][r][ck][8], rounded as the packed
// images are (f2us); FLIP stores tap K*K-1-k in k's place; chunks past C get
// zeros.
template <int K, bool FLIP>
DEV_INLINE void dk_stage_weights(const float* __restrict__ w, int chunk0,
                                 int nck, const DkShape& d, float* wl) {
    for (int idx = threadIdx.x; idx < K * K * d.slw * 8; idx += DK_THREADS) {
        const int j = idx & 7, t = idx >> 3;
        const int k2 = (int)fd_div((unsigned)t, d.fslw);
        const int ck = t - k2 * d.slw;
        const int sp = k2 / K, r = k2 - sp * K;
        const int tap = FLIP ? K * K - 1 - (r * K + sp) : r * K + sp;
        float v = 0.f;
        if (ck < nck)
            v = us2f(f2us(w[((long)(chunk0 + ck) * 8 + j) * (K * K) + tap]));
        wl[idx] = v;
    }
}

DEV_INLINE void dk_read_weights8(const float* p, float (&o)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p);
    const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
    #pragma unroll
    for (int j = 0; j < 4; ++j) { o[j] = a[j]; o[4 + j] = b[j]; }
}

// dw_block_join8 of dwconv.hip on buffers carved out of the tile: sums v[j]
// over the block's cb columns for every (chunk, j) of the slice in index
// order; `parts` threads per channel add cpp consecutive columns each, then
// one thread adds the parts.  A value passes cpp + parts additions.
// red: 8 * (DK_THREADS + 8) floats, part: DK_THREADS floats.
template <class F>
DEV_INLINE void dk_block_join8(const float (&v)[8], float* red, float* part,
                               int slw, int cb, F&& emit) {
    const int tid = threadIdx.x;
    const int nch = slw * 8;
    const int parts = min(cb, max(1, DK_THREADS / nch));
    const int cpp = (cb + parts - 1) / parts;
    dk_barrier<false>();        // the tile's / previous join's readers
    #pragma unroll
    for (int j = 0; j < 8; ++j) red[j * (DK_THREADS + 8) + tid] = v[j];
    dk_barrier<false>();
    for (int idx = tid; idx < nch * parts; idx += DK_THREADS) {
        const int pt = idx / nch, c = idx - pt * nch;
        const int ck = c >> 3, j = c & 7;
        const int ce = min(cb, (pt + 1) * cpp);
        float t = 0.f;
        for (int col = pt * cpp; col < ce; ++col)
            t += red[j * (DK_THREADS + 8) + col * slw + ck];
        part[idx] = t;
    }
    dk_barrier<false>();
    for (int c = tid; c < nch; c += DK_THREADS) {
        float t = 0.f;
        for (int pt = 0; pt < parts; ++pt) t += part[pt * nch + c];
        emit(c, t);
    }
}

// ------------------------------------------------------------------ forward ---
// FLIP: the stride-1 dgrad is this kernel over dy with pad' = K - 1 - pad.
// STATS: per-lane fp32 sum / sum of squares of the pre-rounding v, joined per
// block into slab[2][C][gridDim.x] (the layout of conv2d_fwd_stats); every
// block writes its slot, idle lanes add zeros.  The join buffers overlay the
// tile after the last unit's barrier.
template <int K, int STRIDE, bool FLIP, bool BIAS, bool STATS>
__global__ __launch_bounds__(DK_THREADS) NO_PK_F32
void k_dwconvk_fwd(const bf16* __restrict__ x, const float* __restrict__ w,
                   const float* __restrict__ bias, bf16* __restrict__ y,
                   float* __restrict__ slab, DkShape d) {
    using T = DkTile<K, STRIDE>;
    __shared__ __align__(16) bf16 tile[T::ENTRIES * 8];
    __shared__ __align__(16) float wl[K * K * DK_MAX_SLW * 8];
    static_assert(sizeof(bf16) * T::ENTRIES * 8 +
                  sizeof(float) * K * K * DK_MAX_SLW * 8 <= 80 * 1024,
                  "LDS budget: two blocks per CU");
    const int tid = threadIdx.x;
    const int col = (int)fd_div((unsigned)tid, d.fslw), ck = tid - col * d.slw;
    const int chunk0 = blockIdx.y * d.slw;
    const int nck = min(d.slw, d.chunks - chunk0);
    const bool lane_on = col < d.cb && ck < nck;
    const int colc = lane_on ? col : 0;
    const int c0 = (chunk0 + (lane_on ? ck : 0)) * 8;

    dk_stage_weights<K, FLIP>(w, chunk0, nck, d, wl);
    float bv[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = BIAS ? bias[c0 + j] : 0.f;
    unsigned long zaddr = reinterpret_cast<unsigned long>(dk_zero16);
    asm volatile("" : "+s"(zaddr));
    float sum[8] = {}, sq[8] = {};
    const int rowe8 = d.tcols * d.slw * 8;

    for (int u = blockIdx.x; u < d.units; u += gridDim.x) {
        const int t1 = u / d.nct, ct = u - t1 * d.nct;
        const int n = t1 / d.nruns, run = t1 - n * d.nruns;
        const int p0 = run * d.to, q0 = ct * d.cb;
        const int nrows = min(d.to, d.rows - p0);
        const int q = q0 + col;
        const bool on = lane_on && q < d.cols;
        dk_stage(x + (long)n * d.Hi * d.Wi * d.C + chunk0 * 8,
                 p0 * STRIDE - d.pad, q0 * STRIDE - d.pad, d, nck, tile, zaddr);
        dk_barrier<true>();   // lands the tile

        float acc[T::TO][8] = {};
        #pragma unroll 1
        for (int sp = 0; sp < K; ++sp) {
            float wr[K][8];
            #pragma unroll
            for (int r = 0; r < K; ++r)
                dk_read_weights8(wl + ((sp * K + r) * d.slw + ck) * 8, wr[r]);
            const bf16* tp = tile + ((colc * STRIDE + sp) * d.slw + ck) * 8;
            #pragma unroll
            for (int j = 0; j < T::TROWS; ++j) {
                if (j < d.trows) {
                    const dk_bf16x8 raw =
                        *reinterpret_cast<const dk_bf16x8*>(tp + j * rowe8);
                    float xv[8];
                    #pragma unroll
                    for (int i = 0; i < 8; ++i)
                        xv[i] = us2f((unsigned short)raw[i]);
                    #pragma unroll
                    for (int t = 0; t < T::TO; ++t) {
                        const int r = j - t * STRIDE;
                        if (r >= 0 && r < K) {
                            #pragma unroll
                            for (int i = 0; i < 8; ++i)
                                acc[t][i] = fmaf(xv[i], wr[r][i], acc[t][i]);
                        }
                    }
                }
            }
        }
        bf16* yn = y + (long)n * d.Ho * d.Wo * d.C + c0;
        #pragma unroll
        for (int t = 0; t < T::TO; ++t) {
            if (t < nrows) {
                dk_bf16x8 o;
                #pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float v = acc[t][i];
                    if (BIAS) v += bv[i];
                    if (STATS) {
                        const float vs = on ? v : 0.f;
                        sum[i] += vs;
                        sq[i] = fmaf(vs, vs, sq[i]);
                    }
                    o[i] = dk_f2bf_bits(v);
                }
                if (on)
                    *reinterpret_cast<dk_bf16x8*>(
                        yn + ((long)(p0 + t) * d.Wo + q) * d.C) = o;
            }
        }
        dk_barrier<false>();  // the tile's readers, before the next unit's DMA
    }
    if constexpr (STATS) {
        float* red = reinterpret_cast<float*>(tile);
        float* part = red + 8 * (DK_THREADS + 8);
        const int cbase = chunk0 * 8;
        dk_block_join8(sum, red, part, d.slw, d.cb, [&](int c, float t) {
            if (cbase + c < d.C)
                slab[(long)(cbase + c) * gridDim.x + blockIdx.x] = t;
        });
        dk_block_join8(sq, red, part, d.slw, d.cb, [&](int c, float t) {
            if (cbase + c < d.C)
                slab[((long)d.C + cbase + c) * gridDim.x + blockIdx.x] = t;
        });
    }
}

// ---------------------------------------------------------- dgrad, stride 2 ---
// dx[h][w] = sum over the taps (r, s) with h + pad - r and w + pad - s even
// of dy[(h + pad - r) / 2][(w + pad - s) / 2] * w[r][s].  In padded
// coordinates a = h + pad, b = w + pad the four pixels a in {2i, 2i + 1},
// b in {2j, 2j + 1} read only the 3x3 window dy[i-2 .. i][j-2 .. j]: an even
// coordinate pairs dy[i - l] with tap 2l (l = 0, 1, 2), an odd one with tap
// 2l + 1 (l = 0, 1).  9 + 6 + 6 + 4 = 25 MACs, no zero tap multiplied.
// A lane owns the 2x2 cells (i0 .. i0 + to, j) of one chunk: to x 4 x 8
// accumulators.  The tile is dy rows i0 - 2 .. i0 + to - 1, columns
// j0 - 2 .. j0 + cb - 1, staged as in the forward; the passes go over the
// kernel column s (weights [s][0..4] in registers), which fixes the dy
// column j - s/2 and the parity s & 1 of the dx column.  The cells
// i = 0 .. (H-1+pad)/2, j = 0 .. (W-1+pad)/2 tile dx exactly, so every dx
// pixel is written once — a trailing row or column no output reads gets its
// zeros here.
template <int K>
__global__ __launch_bounds__(DK_THREADS) NO_PK_F32
void k_dwconvk_dgrad_s2(const bf16* __restrict__ dy,
                        const float* __restrict__ w, bf16* __restrict__ dx,
                        DkShape d) {
    static_assert(K == 5, "the 2x2 cell / 3x3 window split is the 5x5's");
    constexpr int TO = DK_CELL_TO, TROWS = TO + 2;
    __shared__ __align__(16) bf16 tile[
        (TROWS * (256 + 2 * DK_MAX_SLW) + 63) / 64 * 64 * 8];
    __shared__ __align__(16) float wl[K * K * DK_MAX_SLW * 8];
    const int tid = threadIdx.x;
    const int col = (int)fd_div((unsigned)tid, d.fslw), ck = tid - col * d.slw;
    const int chunk0 = blockIdx.y * d.slw;
    const int nck = min(d.slw, d.chunks - chunk0);
    const bool lane_on = col < d.cb && ck < nck;
    const int colc = lane_on ? col : 0;
    const int c0 = (chunk0 + (lane_on ? ck : 0)) * 8;

    dk_stage_weights<K, false>(w, chunk0, nck, d, wl);
    unsigned long zaddr = reinterpret_cast<unsigned long>(dk_zero16);
    asm volatile("" : "+s"(zaddr));
    const int rowe8 = d.tcols * d.slw * 8;

    for (int u = blockIdx.x; u < d.units; u += gridDim.x) {
        const int t1 = u / d.nct, ct = u - t1 * d.nct;
        const int n = t1 / d.nruns, run = t1 - n * d.nruns;
        const int i0 = run * d.to, j0 = ct * d.cb;
        const int ncells = min(d.to, d.rows - i0);
        const int jc = j0 + col;
        const bool on = lane_on && jc < d.cols;
        dk_stage(dy + (long)n * d.Hi * d.Wi * d.C + chunk0 * 8, i0 - 2, j0 - 2,
                 d, nck, tile, zaddr);
        dk_barrier<true>();   // lands the tile

        float acc[TO][2][2][8] = {};
        #pragma unroll
        for (int s = 0; s < K; ++s) {
            const int m = s >> 1, b = s & 1;
            float wr[K][8];
            #pragma unroll
            for (int r = 0; r < K; ++r)
                dk_read_weights8(wl + ((s * K + r) * d.slw + ck) * 8, wr[r]);
            const bf16* tp = tile + ((colc + 2 - m) * d.slw + ck) * 8;
            #pragma unroll
            for (int jj = 0; jj < TROWS; ++jj) {
                if (jj < d.trows) {
                    const dk_bf16x8 raw =
                        *reinterpret_cast<const dk_bf16x8*>(tp + jj * rowe8);
                    float g[8];
                    #pragma unroll
                    for (int i = 0; i < 8; ++i)
                        g[i] = us2f((unsigned short)raw[i]);
                    #pragma unroll
                    for (int t = 0; t < TO; ++t) {
                        const int l = t + 2 - jj;   // dy row i - l
                        if (l >= 0 && l <= 2) {
                            #pragma unroll
                            for (int i = 0; i < 8; ++i)
                                acc[t][0][b][i] = fmaf(g[i], wr[2 * l][i],
                                                       acc[t][0][b][i]);
                            if (l <= 1) {
                                #pragma unroll
                                for (int i = 0; i < 8; ++i)
                                    acc[t][1][b][i] = fmaf(
                                        g[i], wr[2 * l + 1][i],
                                        acc[t][1][b][i]);
                            }
                        }
                    }
                }
            }
        }
        bf16* dxn = dx + (long)n * d.Ho * d.Wo * d.C + c0;
        const int wx = 2 * jc - d.pad;
        #pragma unroll
        for (int t = 0; t < TO; ++t) {
            if (t < ncells) {
                #pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const int h = 2 * (i0 + t) + a - d.pad;
                    const bool hok = on && h >= 0 && h < d.Ho;
                    #pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        dk_bf16x8 o;
                        #pragma unroll
                        for (int i = 0; i < 8; ++i)
                            o[i] = dk_f2bf_bits(acc[t][a][b][i]);
                        if (hok && wx + b >= 0 && wx + b < d.Wo)
                            *reinterpret_cast<dk_bf16x8*>(
                                dxn + ((long)h * d.Wo + wx + b) * d.C) = o;
                    }
                }
            }
        }
        dk_barrier<false>();  // the tile's readers, before the next unit's DMA
    }
}

// -------------------------------------------------------------------- wgrad ---
DEV_INLINE dk_bf16x8 dk_load(const bf16* row, bool ok, int colidx, int C) {
    dk_bf16x8 v = {};
    if (ok) v = *reinterpret_cast<const dk_bf16x8*>(row + (long)colidx * C);
    return v;
}

// dw[c][r][s] = sum over (n, p, q) of dy[n][p][q][c] * x[n][p*S-pad+r][q*S-pad+s][c].
// K*K*8 persistent accumulators per lane do not fit, so the tap rows go onto
// lanes: tid = (t * K + r) * slw + ck.  A lane owns (chunk, kernel row r, one
// output row t of the unit's group of `to` = 256 / (K slw) rows) and keeps
// K x 8 accumulators for its taps (r, 0 .. K-1) over all of the block's units
// (image, row group).  It walks along the columns of its output row with a
// sliding K-wide window of converted x chunks in registers; the walk is
// unrolled by K so the slot (S q + s) % K is a compile-time index.  A step
// loads S new x chunks and one dy chunk, issued one step ahead by plain 16 B
// global loads: the K lanes of one (t, chunk) read the same dy address in one
// wave instruction and neighbouring (t, r) pairs the same x rows, which is
// left to the coalescer and the vector L1.  LDS serves the joins only.  With
// DB every lane adds dy up and the r = 0 lanes' sums are joined.  Per tap a
// fixed-order join over t writes slab[block][K*K (+1)][C].
template <int K, int STRIDE, bool DB>
__global__ __launch_bounds__(DK_THREADS) NO_PK_F32
void k_dwconvk_wgrad(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                     float* __restrict__ slab, DkShape d) {
    __shared__ float red[DK_THREADS * 8];
    const int tid = threadIdx.x;
    const int krs = K * d.slw;
    const int t = tid / krs, trem = tid - t * krs;
    const int r = (int)fd_div((unsigned)trem, d.fslw), ck = trem - r * d.slw;
    const int chunk0 = blockIdx.y * d.slw;
    const int nck = min(d.slw, d.chunks - chunk0);
    const bool lane_on = t < d.to && ck < nck;
    const int c0 = (chunk0 + (lane_on ? ck : 0)) * 8;

    float acc[K][8] = {}, dba[8] = {};
    for (int u = blockIdx.x; u < d.units; u += gridDim.x) {
        const int n = u / d.nruns, rg = u - n * d.nruns;
        const int p = rg * d.to + t;
        const bool on = lane_on && p < d.rows;
        const int ih = p * STRIDE - d.pad + r;
        const bool rok = on && ih >= 0 && ih < d.Hi;
        const bf16* xrow = x + (((long)n * d.Hi + (rok ? ih : 0)) * d.Wi) * d.C
                           + c0;
        const bf16* dyrow = dy + (((long)n * d.Ho + (on ? p : 0)) * d.Wo) * d.C
                            + c0;
        float win[K][8];
        #pragma unroll
        for (int s = 0; s < K - STRIDE; ++s) {
            const int iw = s - d.pad;
            const dk_bf16x8 raw = dk_load(xrow, rok && iw >= 0 && iw < d.Wi, iw, d.C);
            #pragma unroll
            for (int i = 0; i < 8; ++i)
                win[s][i] = us2f((unsigned short)raw[i]);
        }
        dk_bf16x8 nx[STRIDE], ng;
        #pragma unroll
        for (int i = 0; i < STRIDE; ++i) {
            const int iw = K - STRIDE + i - d.pad;
            nx[i] = dk_load(xrow, rok && iw >= 0 && iw < d.Wi, iw, d.C);
        }
        ng = dk_load(dyrow, on, 0, d.C);
        for (int qb = 0; qb < d.cols; qb += K) {
            #pragma unroll
            for (int qq = 0; qq < K; ++qq) {
                const int q = qb + qq;
                if (q < d.cols) {
                    float g[8];
                    #pragma unroll
                    for (int i = 0; i < 8; ++i)
                        g[i] = us2f((unsigned short)ng[i]);
                    #pragma unroll
                    for (int a = 0; a < STRIDE; ++a)
                        #pragma unroll
                        for (int i = 0; i < 8; ++i)
                            win[(STRIDE * qq + K - STRIDE + a) % K][i] =
                                us2f((unsigned short)nx[a][i]);
                    // the next step's operands, in flight over the FMAs
                    const bool more = q + 1 < d.cols;
                    #pragma unroll
                    for (int a = 0; a < STRIDE; ++a) {
                        const int iw = (q + 1) * STRIDE + K - STRIDE + a
                                       - d.pad;
                        nx[a] = dk_load(xrow, rok && more && iw >= 0 &&
                                        iw < d.Wi, iw, d.C);
                    }
                    ng = dk_load(dyrow, on && more, q + 1, d.C);
                    #pragma unroll
                    for (int s = 0; s < K; ++s)
                        #pragma unroll
                        for (int i = 0; i < 8; ++i)
                            acc[s][i] = fmaf(g[i],
                                             win[(STRIDE * qq + s) % K][i],
                                             acc[s][i]);
                    if (DB) {
                        #pragma unroll
                        for (int i = 0; i < 8; ++i) dba[i] += g[i];
                    }
                }
            }
        }
    }
    constexpr int KK = K * K + (DB ? 1 : 0);
    float* mine = slab + (long)blockIdx.x * KK * d.C;
    #pragma unroll
    for (int s = 0; s < K; ++s) {
        dk_barrier<false>();                // the previous join's readers
        #pragma unroll
        for (int i = 0; i < 8; ++i) red[tid * 8 + i] = acc[s][i];
        dk_barrier<false>();
        for (int idx = tid; idx < krs * 8; idx += DK_THREADS) {
            const int i = idx & 7, rc = idx >> 3;       // rc = r * slw + ck
            const int rr = (int)fd_div((unsigned)rc, d.fslw);
            const int cki = rc - rr * d.slw;
            float v = 0.f;
            for (int tt = 0; tt < d.to; ++tt) v += red[(tt * krs + rc) * 8 + i];
            if (cki < nck)
                mine[(long)(rr * K + s) * d.C + (chunk0 + cki) * 8 + i] = v;
        }
    }
    if constexpr (DB) {
        dk_barrier<false>();
        #pragma unroll
        for (int i = 0; i < 8; ++i) red[tid * 8 + i] = dba[i];
        dk_barrier<false>();
        for (int idx = tid; idx < d.slw * 8; idx += DK_THREADS) {
            const int i = idx & 7, cki = idx >> 3;      // the r = 0 lanes
            float v = 0.f;
            for (int tt = 0; tt < d.to; ++tt) v += red[(tt * krs + cki) * 8 + i];
            if (cki < nck)
                mine[(long)(K * K) * d.C + (chunk0 + cki) * 8 + i] = v;
        }
    }
}

// slab[S][total] summed over s in fixed order, total = (K*K or K*K + 1) * C
// and i = k * C + c, as k_dwconv3_wgrad_combine: FINAL writes dw[c][k]
// (torch [C,1,K,K]) and db[c] from the whole depth; otherwise block row
// blockIdx.y sums slices [y*CH, y*CH + CH) into out[y][i] (stage 1 of a deep
// slab).  Two chains, even / odd slices, keep two loads in flight.
template <bool FINAL>
__global__ void k_dwconvk_wgrad_combine(const float* __restrict__ slab, int S,
                                        int CH, long total, int C, int K2,
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
        if (k < K2) out[(long)c * K2 + k] = v;
        else db[c] = v;
    }
}

// -------------------------------------------------------------------- hosts ---

enum DkOp { DK_FWD = 0, DK_DGRAD = 1, DK_WGRAD = 2 };

struct DkPlan {
    DkShape d;
    int gx, gy;
};

// The one place that decides slice width, run height, tile and grid; pure
// host arithmetic on the shape under the LDS budget.  (N, C, H, W) is always
// the conv's input x.  to: -1 automatic, else the run height (benchmarks and
// tests), capped by what the kernel's tile holds.
//   * slw = min(C/8, 16), gy = ceil(C/8 / slw), cb = 256 / slw.
//   * fwd / stride-1 dgrad: at most TO = 8 (K5 s1), 4 (K7 s1), 2 (K5 s2) rows
//     per run — what keeps tile + weights <= 80 KiB at slw = 16 — split
//     evenly over the fewest runs (28 rows -> 4 x 7, not 3 x 8 + 4).
//   * stride-2 dgrad: runs of at most 2 cell rows (4 dx rows).
//   * wgrad: to = 256 / (K slw) output rows per group, units = N groups.
//   * gx: fwd / dgrad min(units, DK_MAX_BLOCKS); wgrad units / 4 (a block's
//     K joins want some rows to amortise over) up to DK_WGRAD_MAX_BLOCKS.
static DkPlan dk_plan(DkOp op, long N, long C, long H, long W, long K,
                      long stride, long pad, long to) {
    TORCH_CHECK(N >= 1 && C >= 8 && C % 8 == 0, "dwconvk2d: C must be a "
                "positive multiple of 8; got N=", N, " C=", C);
    TORCH_CHECK((K == 5 && (stride == 1 || stride == 2)) ||
                (K == 7 && stride == 1),
                "dwconvk2d: (kernel, stride) must be (5,1), (5,2) or (7,1); "
                "got (", K, ",", stride, ")");
    TORCH_CHECK(pad >= 0 && pad <= K / 2, "dwconvk2d: padding must be 0 .. ",
                K / 2, "; got ", pad);
    TORCH_CHECK(H + 2 * pad >= K && W + 2 * pad >= K,
                "dwconvk2d: input smaller than the ", K, "x", K, " window");
    TORCH_CHECK(to == -1 || to >= 1, "dwconvk2d: to must be -1 or positive");
    const long P = (H + 2 * pad - K) / stride + 1;
    const long Q = (W + 2 * pad - K) / stride + 1;
    TORCH_CHECK(H <= (1 << 24) && W <= (1 << 24) && C <= (1 << 24) &&
                N * H * W < INT_MAX, "dwconvk2d: index range");
    DkShape d;
    d.N = (int)N; d.C = (int)C; d.chunks = d.C / 8;
    d.pad = (int)pad;
    d.slw = std::min(d.chunks, DK_MAX_SLW);
    d.fslw.init((unsigned)d.slw);
    d.cb = DK_THREADS / d.slw;
    int tomax;
    if (op == DK_WGRAD) {
        d.Hi = (int)H; d.Wi = (int)W; d.Ho = (int)P; d.Wo = (int)Q;
        d.rows = d.Ho; d.cols = d.Wo;
        tomax = DK_THREADS / ((int)K * d.slw);
        d.to = std::min<long>(to > 0 ? std::min<long>(to, tomax) : tomax,
                              d.rows);
        d.trows = d.tcols = 0;
        d.nct = 1;
    } else if (op == DK_DGRAD && stride == 2) {
        d.Hi = (int)P; d.Wi = (int)Q; d.Ho = (int)H; d.Wo = (int)W;
        d.rows = (int)((H - 1 + pad) / 2 + 1);
        d.cols = (int)((W - 1 + pad) / 2 + 1);
        tomax = DK_CELL_TO;
        d.to = std::min<long>(to > 0 ? std::min<long>(to, tomax) : tomax,
                              d.rows);
        d.trows = d.to + 2; d.tcols = d.cb + 2;
        d.nct = ceil_div_i(d.cols, d.cb);
    } else {
        if (op == DK_DGRAD) {
            d.Hi = (int)P; d.Wi = (int)Q; d.Ho = (int)H; d.Wo = (int)W;
            d.pad = (int)(K - 1 - pad);
        } else {
            d.Hi = (int)H; d.Wi = (int)W; d.Ho = (int)P; d.Wo = (int)Q;
        }
        d.rows = d.Ho; d.cols = d.Wo;
        tomax = stride == 2 ? 2 : (K == 5 ? 8 : 4);
        d.to = to > 0 ? (int)std::min<long>(std::min<long>(to, tomax), d.rows)
                      : ceil_div_i(d.rows, ceil_div_i(d.rows, tomax));
        const int s = op == DK_DGRAD ? 1 : (int)stride;
        d.trows = (d.to - 1) * s + (int)K;
        d.tcols = (d.cb - 1) * s + (int)K;
        d.nct = ceil_div_i(d.cols, d.cb);
    }
    d.nruns = ceil_div_i(d.rows, d.to);
    const long units = N * d.nruns * d.nct;
    TORCH_CHECK(units < INT_MAX, "dwconvk2d: too many work units");
    d.units = (int)units;
    DkPlan pl;
    pl.d = d;
    pl.gy = ceil_div_i(d.chunks, d.slw);
    long gx = std::min<long>(units, DK_MAX_BLOCKS);
    if (op == DK_WGRAD)
        gx = std::max<long>(1, std::min<long>(DK_WGRAD_MAX_BLOCKS,
                                              units / DK_WGRAD_UNITS));
    pl.gx = (int)gx;
    return pl;
}

std::tuple<long, long, long, long> dwconvk2d_plan(std::string op, long N,
                                                  long C, long H, long W,
                                                  long K, long stride,
                                                  long pad, long to) {
    DkOp o;
    if (op == "fwd") o = DK_FWD;
    else if (op == "dgrad") o = DK_DGRAD;
    else if (op == "wgrad") o = DK_WGRAD;
    else TORCH_CHECK(false, "dwconvk2d_plan: op must be 'fwd', 'dgrad' or "
                     "'wgrad'; got '", op, "'");
    DkPlan pl = dk_plan(o, N, C, H, W, K, stride, pad, to);
    return {pl.d.slw, pl.d.to, pl.gx, pl.gy};
}

static void dk_check_act(const at::Tensor& t, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                t.dim() == 4, "dwconvk2d: ", what, " must be bf16 [N,C,H,W]");
    TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast),
                "dwconvk2d: ", what, " must be channels_last");
}

static long dk_check_weight(const at::Tensor& w, long C) {
    TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat && w.dim() == 4 &&
                w.is_contiguous() && w.size(0) == C && w.size(1) == 1 &&
                w.size(2) == w.size(3) && (w.size(2) == 5 || w.size(2) == 7),
                "dwconvk2d: w must be the contiguous fp32 [C,1,K,K], K = 5 "
                "or 7");
    return w.size(2);
}

static at::Tensor dk_empty_nhwc(const at::Tensor& like, long n, long c, long h,
                                long w) {
    return at::empty({n, c, h, w}, like.options().memory_format(
        at::MemoryFormat::ChannelsLast));
}

template <int K, int STRIDE, bool FLIP>
static void dk_launch_fwd(const DkPlan& pl, bool hb, bool stats,
                          const at::Tensor& x, const at::Tensor& w,
                          const float* bias, at::Tensor& y, float* slab) {
    auto kern = stats
        ? (hb ? k_dwconvk_fwd<K, STRIDE, FLIP, true, true>
              : k_dwconvk_fwd<K, STRIDE, FLIP, false, true>)
        : (hb ? k_dwconvk_fwd<K, STRIDE, FLIP, true, false>
              : k_dwconvk_fwd<K, STRIDE, FLIP, false, false>);
    hipLaunchKernelGGL(kern, dim3(pl.gx, pl.gy), dim3(DK_THREADS), 0,
                       at::hip::getCurrentHIPStream().stream(),
                       reinterpret_cast<const bf16*>(x.data_ptr()),
                       w.data_ptr<float>(), bias,
                       reinterpret_cast<bf16*>(y.data_ptr()), slab, pl.d);
    HIP_CHECK_LAST();
}

// x: bf16 [N,C,H,W] channels_last; w: the fp32 master [C,1,K,K].  Returns
// (y, slab); slab is the [2][C][gx] BN partial slab with want_stats, else
// undefined.
std::tuple<at::Tensor, at::Tensor> dwconvk2d_fwd(
        at::Tensor x, at::Tensor w, c10::optional<at::Tensor> bias,
        long stride, long pad, bool want_stats, long to) {
    dk_check_act(x, "x");
    const long K = dk_check_weight(w, x.size(1));
    if (bias.has_value())
        TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == at::kFloat &&
                    bias->is_contiguous() && bias->numel() == x.size(1),
                    "dwconvk2d_fwd: bias must be fp32 [C]");
    DkPlan pl = dk_plan(DK_FWD, x.size(0), x.size(1), x.size(2), x.size(3), K,
                        stride, pad, to);
    auto y = dk_empty_nhwc(x, pl.d.N, pl.d.C, pl.d.Ho, pl.d.Wo);
    at::Tensor slab;
    if (want_stats)
        slab = at::empty({2, (long)pl.d.C, (long)pl.gx},
                         x.options().dtype(at::kFloat));
    const float* bp = bias.has_value() ? bias->data_ptr<float>() : nullptr;
    float* sp = want_stats ? slab.data_ptr<float>() : nullptr;
    const bool hb = bias.has_value();
    if (K == 7)
        dk_launch_fwd<7, 1, false>(pl, hb, want_stats, x, w, bp, y, sp);
    else if (stride == 1)
        dk_launch_fwd<5, 1, false>(pl, hb, want_stats, x, w, bp, y, sp);
    else
        dk_launch_fwd<5, 2, false>(pl, hb, want_stats, x, w, bp, y, sp);
    return {y, slab};
}

// dy: bf16 [N,C,P,Q] channels_last of the conv over an [N,C,H,W] input.
// Stride 1 is the forward kernel with flipped taps and pad K - 1 - pad;
// stride 2 the 2x2-cell kernel.  Every dx element is written by the kernel.
at::Tensor dwconvk2d_dgrad(at::Tensor dy, at::Tensor w, long H, long W,
                           long stride, long pad, long to) {
    dk_check_act(dy, "dy");
    const long K = dk_check_weight(w, dy.size(1));
    TORCH_CHECK(H >= 1 && W >= 1, "dwconvk2d_dgrad: bad H / W");
    DkPlan pl = dk_plan(DK_DGRAD, dy.size(0), dy.size(1), H, W, K, stride,
                        pad, to);
    TORCH_CHECK(dy.size(2) == pl.d.Hi && dy.size(3) == pl.d.Wi,
                "dwconvk2d_dgrad: dy is not the output of this conv over "
                "[H, W] = [", H, ", ", W, "]");
    auto dx = dk_empty_nhwc(dy, pl.d.N, pl.d.C, H, W);
    if (stride == 1) {
        if (K == 7)
            dk_launch_fwd<7, 1, true>(pl, false, false, dy, w, nullptr, dx,
                                      nullptr);
        else
            dk_launch_fwd<5, 1, true>(pl, false, false, dy, w, nullptr, dx,
                                      nullptr);
    } else {
        hipLaunchKernelGGL(k_dwconvk_dgrad_s2<5>, dim3(pl.gx, pl.gy),
                           dim3(DK_THREADS), 0,
                           at::hip::getCurrentHIPStream().stream(),
                           reinterpret_cast<const bf16*>(dy.data_ptr()),
                           w.data_ptr<float>(),
                           reinterpret_cast<bf16*>(dx.data_ptr()), pl.d);
        HIP_CHECK_LAST();
    }
    return dx;
}

// Returns (dw fp32 [C,1,K,K], db fp32 [C]); db is undefined without want_db.
std::tuple<at::Tensor, at::Tensor> dwconvk2d_wgrad(at::Tensor dy, at::Tensor x,
                                                   long K, long stride,
                                                   long pad, bool want_db,
                                                   long to) {
    dk_check_act(dy, "dy");
    dk_check_act(x, "x");
    DkPlan pl = dk_plan(DK_WGRAD, x.size(0), x.size(1), x.size(2), x.size(3),
                        K, stride, pad, to);
    TORCH_CHECK(dy.size(0) == x.size(0) && dy.size(1) == x.size(1) &&
                dy.size(2) == pl.d.Ho && dy.size(3) == pl.d.Wo,
                "dwconvk2d_wgrad: dy is not the output of this conv over x");
    const long C = pl.d.C, K2 = K * K, KK = K2 + (want_db ? 1 : 0);
    const long total = KK * C;
    auto fopt = x.options().dtype(at::kFloat);
    auto slab = at::empty({(long)pl.gx, KK, C}, fopt);
    auto dw = at::empty({C, 1, K, K}, fopt);
    at::Tensor db;
    if (want_db) db = at::empty({C}, fopt);
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto kern = K == 7
        ? (want_db ? k_dwconvk_wgrad<7, 1, true> : k_dwconvk_wgrad<7, 1, false>)
        : stride == 1
        ? (want_db ? k_dwconvk_wgrad<5, 1, true> : k_dwconvk_wgrad<5, 1, false>)
        : (want_db ? k_dwconvk_wgrad<5, 2, true> : k_dwconvk_wgrad<5, 2, false>);
    hipLaunchKernelGGL(kern, dim3(pl.gx, pl.gy), dim3(DK_THREADS), 0, stream,
                       reinterpret_cast<const bf16*>(dy.data_ptr()),
                       reinterpret_cast<const bf16*>(x.data_ptr()),
                       slab.data_ptr<float>(), pl.d);
    HIP_CHECK_LAST();
    const int cgx = ceil_div_i(total, 256);
    const float* src = slab.data_ptr<float>();
    int S = pl.gx;
    at::Tensor slab2;
    if (S > DK_COMBINE_DIRECT) {
        const int nch = ceil_div_i(S, DK_COMBINE_CH);
        slab2 = at::empty({(long)nch, total}, fopt);
        hipLaunchKernelGGL(k_dwconvk_wgrad_combine<false>, dim3(cgx, nch),
                           dim3(256), 0, stream, src, S, DK_COMBINE_CH, total,
                           (int)C, (int)K2, slab2.data_ptr<float>(),
                           (float*)nullptr);
        HIP_CHECK_LAST();
        src = slab2.data_ptr<float>();
        S = nch;
    }
    hipLaunchKernelGGL(k_dwconvk_wgrad_combine<true>, dim3(cgx, 1), dim3(256),
                       0, stream, src, S, S, total, (int)C, (int)K2,
                       dw.data_ptr<float>(),
                       want_db ? db.data_ptr<float>() : nullptr);
    HIP_CHECK_LAST();
    return {dw, db};
}
