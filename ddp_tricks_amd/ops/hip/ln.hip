// ln.hip — the three elementwise pieces of a ConvNeXt block over bf16
// channels_last activations:
//
//   LayerNorm over the C channels of one pixel   y = (x - mean) rstd gamma + beta
//   GELU, exact erf form                         a = z/2 (1 + erf(z / sqrt 2))
//   layer scale with the residual add            y = resid + gamma_c u
//
// and their backward passes.  An activation [N, C, H, W] is a matrix of
// M = N*H*W rows of C bf16, and LayerNorm's statistics are per ROW — nothing
// of bn.hip's per-channel or gn.hip's per-(image, group) three-pass split
// fits.  A row fits in the registers of a few lanes, so LayerNorm is one pass:
//
//   * a row belongs to lpr lanes of one wave, lpr the smallest power of two
//     >= C/8 capped at 64; lane `sub` of the row holds the 16 B chunks
//     sub + j * lpr, j < CPL (a template parameter, 1 / 2 / 4), so the loads of
//     a wave are contiguous runs;
//   * a wave carries 64 / lpr rows, a block of 256 a "row group" of
//     rpg = 256 / lpr rows; thread t owns row t / lpr of its group (that is
//     wave * (64 / lpr) + slot) and sub = t % lpr;
//   * block b walks the groups b, b + gridDim.x, ...; the 16 B loads of the
//     next group are issued before the arithmetic of the current one;
//   * chunk slots past C/8 and rows past M load zeros and store nothing.  The
//     variance masks them explicitly: a dead slot must not add (0 - mean)^2;
//   * the row sums go through an xor-shuffle tree over the lpr lanes, every
//     lane ends with the same bits;
//   * a lane's gamma / beta (8 * CPL each) are read once per block from the
//     fp32 master parameters.
//
// The backward keeps dgamma / dbeta in 16 * CPL fp32 registers per lane over
// all of the block's rows, joins the lanes that hold the same chunk through
// LDS in a fixed order (row of the group, i.e. slot within the wave, then
// wave) and writes slab[block][2][C]; k_ln_combine adds the blocks in double.
// Layer scale uses the same lane-to-chunk mapping without the tree, and the
// same join and combine for its dgamma.  GELU is flat over 16 B chunks.
// No atomics, no grid that depends on the device, zero scratch.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

constexpr int LN_BLOCK = 256;
constexpr int LN_MAX_C = 2048;
constexpr int LN_BWD_GRID = 512;   // cap of the slab depth (backward grids)
constexpr int LN_FWD_GRID = 2048;  // cap of the forward grids: 8 blocks a CU
constexpr int LN_CQ = 16;          // combine: interleaved chains per column
constexpr int GELU_GRID = 2048;

struct LnPlan { int lpr, cpl, rpg, grid, groups; };

// The one host decision, a function of (M, C) alone.  grid is the backward's
// (the slab depth); the forwards use up to LN_FWD_GRID blocks.  blocks > 0
// forces both, clamped to the number of row groups.
static LnPlan ln_make_plan(long M, long C, long blocks, bool fwd = false) {
    TORCH_CHECK(C >= 8 && C % 8 == 0 && C <= LN_MAX_C,
                "ln2d: needs C % 8 == 0 and C <= ", LN_MAX_C, ", got C = ", C);
    // (row indices are ints, and the walk forms row + grid * rpg <= row + 2^19)
    TORCH_CHECK(M >= 1 && M < (1l << 31) - (1l << 20),
                "ln2d: needs 1 <= N*H*W < 2^31 - 2^20");
    LnPlan p;
    const int chunks = (int)(C / 8);
    p.lpr = 1;
    while (p.lpr < chunks && p.lpr < 64) p.lpr *= 2;
    const int need = (chunks + p.lpr - 1) / p.lpr;
    p.cpl = need <= 1 ? 1 : need <= 2 ? 2 : 4;
    p.rpg = LN_BLOCK / p.lpr;
    p.groups = (int)((M + p.rpg - 1) / p.rpg);
    const long cap = blocks > 0 ? blocks : fwd ? LN_FWD_GRID : LN_BWD_GRID;
    p.grid = (int)std::min<long>(cap, p.groups);
    return p;
}

std::tuple<long, long, long, long> ln2d_plan(long M, long C, long blocks) {
    LnPlan p = ln_make_plan(M, C, blocks);
    return {p.lpr, p.cpl, p.rpg, p.grid};
}

DEV_INLINE s16x8 ln_ld8(const bf16* p) {
    return *reinterpret_cast<const s16x8*>(p);
}
DEV_INLINE void ln_st8(bf16* p, s16x8 v) {
    *reinterpret_cast<s16x8*>(p) = v;
}

// 8 fp32 -> 8 bf16, round to nearest even, on gfx950's packed conversion
// (v_cvt_pk_bf16_f32: one instruction per pair where the integer sequence of
// f2us takes five per element; the same bits for every finite value)
typedef __bf16 ln_bf16x2 __attribute__((ext_vector_type(2)));
DEV_INLINE s16x8 ln_pack8(const float (&f)[8]) {
    s16x8 o;
    #pragma unroll
    for (int e = 0; e < 8; e += 2) {
        const s16x2 p = __builtin_bit_cast(
            s16x2, __builtin_convertvector(f32x2{f[e], f[e + 1]}, ln_bf16x2));
        o[e] = p[0];
        o[e + 1] = p[1];
    }
    return o;
}

// A lane's place in the split: its row within a group, its first chunk and
// which of its CPL chunk slots exist.
template <int CPL>
struct LnLane {
    int sub, rig;
    bool live[CPL];
};

template <int CPL>
DEV_INLINE LnLane<CPL> ln_lane(int C, int lpr) {
    LnLane<CPL> L;
    L.sub = threadIdx.x & (lpr - 1);
    L.rig = threadIdx.x >> __builtin_ctz(lpr);
    #pragma unroll
    for (int j = 0; j < CPL; ++j) L.live[j] = (L.sub + j * lpr) * 8 < C;
    return L;
}

// the lane's chunks of row `row` of a [M, C] matrix; zeros where the slot or
// the row does not exist
template <int CPL>
DEV_INLINE void ln_load(const LnLane<CPL>& L, const bf16* __restrict__ x,
                        int row, int M, int C, int lpr, s16x8 (&v)[CPL]) {
    const bool ok = row < M;
    const bf16* p = x + (long)row * C + L.sub * 8;
    #pragma unroll
    for (int j = 0; j < CPL; ++j)
        v[j] = ok && L.live[j] ? ln_ld8(p + j * lpr * 8) : s16x8{};
}

template <int CPL>
DEV_INLINE void ln_store(const LnLane<CPL>& L, bf16* __restrict__ y, int row,
                         int M, int C, int lpr, const s16x8 (&v)[CPL]) {
    if (row >= M) return;
    bf16* p = y + (long)row * C + L.sub * 8;
    #pragma unroll
    for (int j = 0; j < CPL; ++j)
        if (L.live[j]) ln_st8(p + j * lpr * 8, v[j]);
}

// the lane's 8 * CPL entries of a fp32 [C] vector; zeros in dead slots
template <int CPL>
DEV_INLINE void ln_load_param(const LnLane<CPL>& L, const float* __restrict__ g,
                              int lpr, float (&out)[CPL][8]) {
    #pragma unroll
    for (int j = 0; j < CPL; ++j) {
        f32x4 a = {}, b = {};
        if (L.live[j]) {
            const f32x4* p =
                reinterpret_cast<const f32x4*>(g + (L.sub + j * lpr) * 8);
            a = p[0];
            b = p[1];
        }
        #pragma unroll
        for (int e = 0; e < 4; ++e) {
            out[j][e] = a[e];
            out[j][4 + e] = b[e];
        }
    }
}

// Sum over the lpr lanes of a row: xor butterfly, widest step first.  lpr is
// a kernel argument, so every `if` is a scalar branch and a step the row does
// not need costs no shuffle.
DEV_INLINE float ln_tree(float v, int lpr) {
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        if (off < lpr) v += __shfl_xor(v, off, 64);
    return v;
}
DEV_INLINE void ln_tree2(float& a, float& b, int lpr) {
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        if (off < lpr) {
            a += __shfl_xor(a, off, 64);
            b += __shfl_xor(b, off, 64);
        }
}

// ---------------------------------------------------- LayerNorm forward -----

template <int CPL, bool SAVE>
__global__ __launch_bounds__(LN_BLOCK)
void k_ln_fwd(const bf16* __restrict__ x, const float* __restrict__ gamma,
              const float* __restrict__ beta, bf16* __restrict__ y,
              float* __restrict__ mean, float* __restrict__ rstd, int M, int C,
              int lpr, int rpg, int groups, float eps) {
    const LnLane<CPL> L = ln_lane<CPL>(C, lpr);
    float gm[CPL][8], bt[CPL][8];
    ln_load_param<CPL>(L, gamma, lpr, gm);
    ln_load_param<CPL>(L, beta, lpr, bt);
    const float fc = (float)C;

    s16x8 cur[CPL], nxt[CPL];
    int g = blockIdx.x;
    ln_load<CPL>(L, x, g * rpg + L.rig, M, C, lpr, cur);
    for (; g < groups; g += gridDim.x) {
        const int row = g * rpg + L.rig;
        const int gn = g + gridDim.x;
        if (gn < groups) ln_load<CPL>(L, x, gn * rpg + L.rig, M, C, lpr, nxt);

        float f[CPL][8];
        float s = 0.f;
        #pragma unroll
        for (int j = 0; j < CPL; ++j)
            #pragma unroll
            for (int e = 0; e < 8; ++e) {
                f[j][e] = us2f((unsigned short)cur[j][e]);
                s += f[j][e];
            }
        const float mu = ln_tree(s, lpr) / fc;
        float q = 0.f;
        #pragma unroll
        for (int j = 0; j < CPL; ++j)
            #pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = L.live[j] ? f[j][e] - mu : 0.f;
                f[j][e] = d;
                q = fmaf(d, d, q);
            }
        const float rs = 1.f / sqrtf(ln_tree(q, lpr) / fc + eps);
        s16x8 o[CPL];
        #pragma unroll
        for (int j = 0; j < CPL; ++j) {
            #pragma unroll
            for (int e = 0; e < 8; ++e)
                f[j][e] = fmaf(f[j][e] * rs, gm[j][e], bt[j][e]);
            o[j] = ln_pack8(f[j]);
        }
        ln_store<CPL>(L, y, row, M, C, lpr, o);
        if (SAVE && L.sub == 0 && row < M) {
            mean[row] = mu;
            rstd[row] = rs;
        }
        #pragma unroll
        for (int j = 0; j < CPL; ++j) cur[j] = nxt[j];
    }
}

// ------------------------------------------------------------ the join -----

// Every lane puts its 8 * CPL accumulators into LDS, one chunk slot at a time;
// thread t then adds, for channel t (and t + 256) of the slot, the rpg lanes
// that hold it in row-of-group order — slot within the wave, then wave — and
// writes out[c] for c < C.  out is one [C] row of the block's slab entry.
template <int CPL>
DEV_INLINE void ln_join(const float (&acc)[CPL][8], float* __restrict__ red,
                        int C, int lpr, int rpg, float* __restrict__ out) {
    const int wc = lpr * 8;                 // channels of one chunk slot
    #pragma unroll
    for (int j = 0; j < CPL; ++j) {
        __syncthreads();
        f32x4* p = reinterpret_cast<f32x4*>(red + threadIdx.x * 8);
        p[0] = f32x4{acc[j][0], acc[j][1], acc[j][2], acc[j][3]};
        p[1] = f32x4{acc[j][4], acc[j][5], acc[j][6], acc[j][7]};
        __syncthreads();
        for (int t = threadIdx.x; t < wc; t += LN_BLOCK) {
            const int c = j * wc + t;
            if (c >= C) break;
            float v = 0.f;
            for (int k = 0; k < rpg; ++k) v += red[k * wc + t];
            out[c] = v;
        }
    }
}

// out[c] = sum over blocks of slab[b][c], c < cols.  16 x 16 threads over
// (q, column): thread q adds blocks q, q + 16, ... in double, the 16 chains
// meet in LDS and are added in q order; one rounding to fp32.
__global__ __launch_bounds__(LN_BLOCK)
void k_ln_combine(const float* __restrict__ slab, int nb, int cols,
                  float* __restrict__ out) {
    __shared__ double red[LN_CQ][LN_CQ];
    const int cl = threadIdx.x & (LN_CQ - 1);
    const int q = threadIdx.x / LN_CQ;
    const int c = blockIdx.x * LN_CQ + cl;
    double a = 0.0;
    if (c < cols)
        for (int i = q; i < nb; i += LN_CQ)
            a += (double)slab[(long)i * cols + c];
    red[q][cl] = a;
    __syncthreads();
    if (q == 0 && c < cols) {
        double t = 0.0;
        #pragma unroll
        for (int w = 0; w < LN_CQ; ++w) t += red[w][cl];
        out[c] = (float)t;
    }
}

// --------------------------------------------------- LayerNorm backward -----

// dx = rstd (g - (s1 + xhat s2) / C), g = dy gamma, s1 = sum g,
// s2 = sum g xhat; s1 / C and s2 / C are formed once per row.
// slab[block][0][c] = dgamma partial, slab[block][1][c] = dbeta partial.
template <int CPL>
__global__ __launch_bounds__(LN_BLOCK)
void k_ln_bwd(const bf16* __restrict__ x, const bf16* __restrict__ dy,
              const float* __restrict__ mean, const float* __restrict__ rstd,
              const float* __restrict__ gamma, bf16* __restrict__ dx,
              float* __restrict__ slab, int M, int C, int lpr, int rpg,
              int groups) {
    __shared__ __attribute__((aligned(16))) float red[LN_BLOCK * 8];
    const LnLane<CPL> L = ln_lane<CPL>(C, lpr);
    float gm[CPL][8];
    ln_load_param<CPL>(L, gamma, lpr, gm);
    const float fc = (float)C;
    float dg[CPL][8] = {}, db[CPL][8] = {};

    s16x8 xc[CPL], gc[CPL], xn[CPL], gn[CPL];
    int g = blockIdx.x;
    int row = g * rpg + L.rig;
    ln_load<CPL>(L, x, row, M, C, lpr, xc);
    ln_load<CPL>(L, dy, row, M, C, lpr, gc);
    float mu = row < M ? mean[row] : 0.f;
    float rs = row < M ? rstd[row] : 0.f;
    for (; g < groups; g += gridDim.x) {
        row = g * rpg + L.rig;
        const int nrow = row + gridDim.x * rpg;
        float mun = 0.f, rsn = 0.f;
        if (g + gridDim.x < groups) {
            ln_load<CPL>(L, x, nrow, M, C, lpr, xn);
            ln_load<CPL>(L, dy, nrow, M, C, lpr, gn);
            if (nrow < M) {
                mun = mean[nrow];
                rsn = rstd[nrow];
            }
        }

        // dead slots and rows hold dy = 0: they add nothing anywhere
        float xh[CPL][8], gg[CPL][8];
        float s1 = 0.f, s2 = 0.f;
        #pragma unroll
        for (int j = 0; j < CPL; ++j)
            #pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = us2f((unsigned short)gc[j][e]);
                xh[j][e] = (us2f((unsigned short)xc[j][e]) - mu) * rs;
                gg[j][e] = d * gm[j][e];
                s1 += gg[j][e];
                s2 = fmaf(gg[j][e], xh[j][e], s2);
                db[j][e] += d;
                dg[j][e] = fmaf(d, xh[j][e], dg[j][e]);
            }
        ln_tree2(s1, s2, lpr);
        const float a1 = s1 / fc, a2 = s2 / fc;
        s16x8 o[CPL];
        #pragma unroll
        for (int j = 0; j < CPL; ++j) {
            #pragma unroll
            for (int e = 0; e < 8; ++e)
                gg[j][e] = rs * (gg[j][e] - fmaf(xh[j][e], a2, a1));
            o[j] = ln_pack8(gg[j]);
        }
        ln_store<CPL>(L, dx, row, M, C, lpr, o);
        #pragma unroll
        for (int j = 0; j < CPL; ++j) {
            xc[j] = xn[j];
            gc[j] = gn[j];
        }
        mu = mun;
        rs = rsn;
    }
    float* mine = slab + (long)blockIdx.x * 2 * C;
    ln_join<CPL>(dg, red, C, lpr, rpg, mine);
    ln_join<CPL>(db, red, C, lpr, rpg, mine + C);
}

// ---------------------------------------------------------- layer scale -----

// y = fma(gamma_c, u, resid)
template <int CPL>
__global__ __launch_bounds__(LN_BLOCK)
void k_lscale_fwd(const bf16* __restrict__ u, const bf16* __restrict__ resid,
                  const float* __restrict__ gamma, bf16* __restrict__ y, int M,
                  int C, int lpr, int rpg, int groups) {
    const LnLane<CPL> L = ln_lane<CPL>(C, lpr);
    float gm[CPL][8];
    ln_load_param<CPL>(L, gamma, lpr, gm);
    s16x8 uc[CPL], rc[CPL], un[CPL], rn[CPL];
    int g = blockIdx.x;
    ln_load<CPL>(L, u, g * rpg + L.rig, M, C, lpr, uc);
    ln_load<CPL>(L, resid, g * rpg + L.rig, M, C, lpr, rc);
    for (; g < groups; g += gridDim.x) {
        const int row = g * rpg + L.rig;
        if (g + gridDim.x < groups) {
            const int nrow = row + gridDim.x * rpg;
            ln_load<CPL>(L, u, nrow, M, C, lpr, un);
            ln_load<CPL>(L, resid, nrow, M, C, lpr, rn);
        }
        s16x8 o[CPL];
        #pragma unroll
        for (int j = 0; j < CPL; ++j) {
            float v[8];
            #pragma unroll
            for (int e = 0; e < 8; ++e)
                v[e] = fmaf(gm[j][e], us2f((unsigned short)uc[j][e]),
                            us2f((unsigned short)rc[j][e]));
            o[j] = ln_pack8(v);
        }
        ln_store<CPL>(L, y, row, M, C, lpr, o);
        #pragma unroll
        for (int j = 0; j < CPL; ++j) {
            uc[j] = un[j];
            rc[j] = rn[j];
        }
    }
}

// du = gamma_c dy; slab[block][c] = sum over the block's rows of dy u
template <int CPL>
__global__ __launch_bounds__(LN_BLOCK)
void k_lscale_bwd(const bf16* __restrict__ dy, const bf16* __restrict__ u,
                  const float* __restrict__ gamma, bf16* __restrict__ du,
                  float* __restrict__ slab, int M, int C, int lpr, int rpg,
                  int groups) {
    __shared__ __attribute__((aligned(16))) float red[LN_BLOCK * 8];
    const LnLane<CPL> L = ln_lane<CPL>(C, lpr);
    float gm[CPL][8];
    ln_load_param<CPL>(L, gamma, lpr, gm);
    float dg[CPL][8] = {};
    s16x8 uc[CPL], gc[CPL], un[CPL], gn[CPL];
    int g = blockIdx.x;
    ln_load<CPL>(L, u, g * rpg + L.rig, M, C, lpr, uc);
    ln_load<CPL>(L, dy, g * rpg + L.rig, M, C, lpr, gc);
    for (; g < groups; g += gridDim.x) {
        const int row = g * rpg + L.rig;
        if (g + gridDim.x < groups) {
            const int nrow = row + gridDim.x * rpg;
            ln_load<CPL>(L, u, nrow, M, C, lpr, un);
            ln_load<CPL>(L, dy, nrow, M, C, lpr, gn);
        }
        s16x8 o[CPL];
        #pragma unroll
        for (int j = 0; j < CPL; ++j) {
            float v[8];
            #pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = us2f((unsigned short)gc[j][e]);
                v[e] = gm[j][e] * d;
                dg[j][e] = fmaf(d, us2f((unsigned short)uc[j][e]), dg[j][e]);
            }
            o[j] = ln_pack8(v);
        }
        ln_store<CPL>(L, du, row, M, C, lpr, o);
        #pragma unroll
        for (int j = 0; j < CPL; ++j) {
            uc[j] = un[j];
            gc[j] = gn[j];
        }
    }
    ln_join<CPL>(dg, red, C, lpr, rpg, slab + (long)blockIdx.x * C);
}

// ----------------------------------------------------------------- GELU -----

// erf by the device library's erff scheme and coefficients (an odd polynomial
// in x below 1, 1 - exp(-p(|x|)) above), with the hardware exp2 in place of
// the library's correctly rounded expf: p >= 0.84, so the fast exp's error,
// about (1.7 p + 2) 2^-24 relative, is below 2 * 2^-24 absolute.  The GELU
// kernels are bound by VALU work, not by HBM, and the library's expf is a
// third of their instructions.
DEV_INLINE float ln_erf(float x) {
    const float a = fabsf(x);
    float r;
    if (a < 1.f) {
        const float t = x * x;
        float q = fmaf(t, -0.000561801775f, 0.00491381623f);
        q = fmaf(t, q, -0.0267075151f);
        q = fmaf(t, q, 0.112800106f);
        q = fmaf(t, q, -0.376122952f);
        q = fmaf(t, q, 0.128379107f);
        r = fmaf(a, q, a);
    } else {
        float q = fmaf(a, 1.69988107e-05f, -0.000378677854f);
        q = fmaf(a, q, 0.00385781587f);
        q = fmaf(a, q, -0.0241816975f);
        q = fmaf(a, q, 0.106668264f);
        q = fmaf(a, q, 0.634933293f);
        q = fmaf(a, q, 0.128689408f);
        r = 1.f - __expf(-fmaf(a, q, a));
    }
    return copysignf(r, x);
}

// flat over the n8 16 B chunks of a dense bf16 tensor
__global__ __launch_bounds__(LN_BLOCK)
void k_gelu_fwd(const bf16* __restrict__ z, bf16* __restrict__ a, long n8) {
    const long step = (long)gridDim.x * LN_BLOCK;
    for (long i = (long)blockIdx.x * LN_BLOCK + threadIdx.x; i < n8;
         i += step) {
        const s16x8 v = ln_ld8(z + i * 8);
        float o[8];
        #pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = us2f((unsigned short)v[e]);
            o[e] = 0.5f * f * (1.f + ln_erf(f * 0.70710678f));
        }
        ln_st8(a + i * 8, ln_pack8(o));
    }
}

// dz = dy (Phi(z) + z phi(z)), Phi = (1 + erf(z / sqrt 2)) / 2,
// phi = exp(-z^2 / 2) / sqrt(2 pi)
__global__ __launch_bounds__(LN_BLOCK)
void k_gelu_bwd(const bf16* __restrict__ dy, const bf16* __restrict__ z,
                bf16* __restrict__ dz, long n8) {
    const long step = (long)gridDim.x * LN_BLOCK;
    for (long i = (long)blockIdx.x * LN_BLOCK + threadIdx.x; i < n8;
         i += step) {
        const s16x8 v = ln_ld8(z + i * 8);
        const s16x8 gv = ln_ld8(dy + i * 8);
        float o[8];
        #pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = us2f((unsigned short)v[e]);
            const float cdf = 0.5f * (1.f + ln_erf(f * 0.70710678f));
            const float pdf = __expf(-0.5f * f * f) * 0.39894228f;
            o[e] = us2f((unsigned short)gv[e]) * fmaf(f, pdf, cdf);
        }
        ln_st8(dz + i * 8, ln_pack8(o));
    }
}

// ---------------------------------------------------------------- hosts -----

static void ln_check_act(const at::Tensor& t, const char* who,
                         const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                t.dim() == 4, who, ": ", what, " must be bf16 [N,C,H,W]");
    TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast),
                who, ": ", what, " must be channels_last");
}

static void ln_check_vec(const at::Tensor& t, long n, const char* who,
                         const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                t.is_contiguous() && t.numel() == n,
                who, ": ", what, " must be contiguous fp32 with ", n,
                " elements");
}

static at::Tensor ln_empty_like(const at::Tensor& x) {
    return at::empty_like(
        x, x.options().memory_format(at::MemoryFormat::ChannelsLast));
}

static const bf16* ln_cptr(const at::Tensor& t) {
    return reinterpret_cast<const bf16*>(t.data_ptr());
}
static bf16* ln_ptr(at::Tensor& t) {
    return reinterpret_cast<bf16*>(t.data_ptr());
}

// launch KERN<CPL>(args...) for the plan's cpl
#define LN_LAUNCH(KERN, P, GRID, STREAM, ...)                                \
    do {                                                                     \
        if ((P).cpl == 1)                                                    \
            hipLaunchKernelGGL((KERN<1>), dim3(GRID), dim3(LN_BLOCK), 0,     \
                               STREAM, __VA_ARGS__);                         \
        else if ((P).cpl == 2)                                               \
            hipLaunchKernelGGL((KERN<2>), dim3(GRID), dim3(LN_BLOCK), 0,     \
                               STREAM, __VA_ARGS__);                         \
        else                                                                 \
            hipLaunchKernelGGL((KERN<4>), dim3(GRID), dim3(LN_BLOCK), 0,     \
                               STREAM, __VA_ARGS__);                         \
        HIP_CHECK_LAST();                                                    \
    } while (0)

static void ln_combine(const at::Tensor& slab, int nb, int cols, float* out,
                       hipStream_t stream) {
    hipLaunchKernelGGL(k_ln_combine, dim3(ceil_div_i(cols, LN_CQ)),
                       dim3(LN_BLOCK), 0, stream, slab.data_ptr<float>(), nb,
                       cols, out);
    HIP_CHECK_LAST();
}

template <int CPL>
static void ln_launch_fwd(bool save, int grid, hipStream_t st, const bf16* x,
                          const float* g, const float* b, bf16* y, float* mean,
                          float* rstd, int M, int C, const LnPlan& p,
                          float eps) {
    if (save)
        hipLaunchKernelGGL((k_ln_fwd<CPL, true>), dim3(grid), dim3(LN_BLOCK),
                           0, st, x, g, b, y, mean, rstd, M, C, p.lpr, p.rpg,
                           p.groups, eps);
    else
        hipLaunchKernelGGL((k_ln_fwd<CPL, false>), dim3(grid), dim3(LN_BLOCK),
                           0, st, x, g, b, y, mean, rstd, M, C, p.lpr, p.rpg,
                           p.groups, eps);
    HIP_CHECK_LAST();
}

// (y, mean [M], rstd [M]); mean and rstd are empty without `save`
std::tuple<at::Tensor, at::Tensor, at::Tensor> ln2d_fwd(
    at::Tensor x, at::Tensor gamma, at::Tensor beta, double eps, bool save,
    long blocks) {
    ln_check_act(x, "ln2d_fwd", "x");
    const long C = x.size(1), M = x.numel() / std::max<long>(C, 1);
    const LnPlan p = ln_make_plan(M, C, blocks, true);
    ln_check_vec(gamma, C, "ln2d_fwd", "gamma");
    ln_check_vec(beta, C, "ln2d_fwd", "beta");
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto fopts = x.options().dtype(at::kFloat);
    auto y = ln_empty_like(x);
    auto mean = at::empty({save ? M : 0}, fopts);
    auto rstd = at::empty({save ? M : 0}, fopts);
    float* mp = save ? mean.data_ptr<float>() : nullptr;
    float* rp = save ? rstd.data_ptr<float>() : nullptr;
    auto run = p.cpl == 1 ? ln_launch_fwd<1>
             : p.cpl == 2 ? ln_launch_fwd<2> : ln_launch_fwd<4>;
    run(save, p.grid, stream, ln_cptr(x), gamma.data_ptr<float>(),
        beta.data_ptr<float>(), ln_ptr(y), mp, rp, (int)M, (int)C, p,
        (float)eps);
    return {y, mean, rstd};
}

// (dx, dgamma, dbeta)
std::tuple<at::Tensor, at::Tensor, at::Tensor> ln2d_bwd(
    at::Tensor x, at::Tensor dy, at::Tensor gamma, at::Tensor mean,
    at::Tensor rstd, long blocks) {
    ln_check_act(x, "ln2d_bwd", "x");
    ln_check_act(dy, "ln2d_bwd", "dy");
    TORCH_CHECK(dy.sizes() == x.sizes(), "ln2d_bwd: dy shape differs from x");
    const long C = x.size(1), M = x.numel() / std::max<long>(C, 1);
    const LnPlan p = ln_make_plan(M, C, blocks);
    ln_check_vec(gamma, C, "ln2d_bwd", "gamma");
    ln_check_vec(mean, M, "ln2d_bwd", "mean");
    ln_check_vec(rstd, M, "ln2d_bwd", "rstd");
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto fopts = x.options().dtype(at::kFloat);
    auto dx = ln_empty_like(x);
    auto slab = at::empty({p.grid, 2, C}, fopts);
    auto dgb = at::empty({2, C}, fopts);
    LN_LAUNCH(k_ln_bwd, p, p.grid, stream, ln_cptr(x), ln_cptr(dy),
              mean.data_ptr<float>(), rstd.data_ptr<float>(),
              gamma.data_ptr<float>(), ln_ptr(dx), slab.data_ptr<float>(),
              (int)M, (int)C, p.lpr, p.rpg, p.groups);
    ln_combine(slab, p.grid, (int)(2 * C), dgb.data_ptr<float>(), stream);
    return {dx, dgb.select(0, 0), dgb.select(0, 1)};
}

// y = resid + gamma_c u
at::Tensor lscale_fwd(at::Tensor u, at::Tensor gamma, at::Tensor resid) {
    ln_check_act(u, "lscale_fwd", "u");
    ln_check_act(resid, "lscale_fwd", "resid");
    TORCH_CHECK(resid.sizes() == u.sizes(),
                "lscale_fwd: resid shape differs from u");
    const long C = u.size(1), M = u.numel() / std::max<long>(C, 1);
    const LnPlan p = ln_make_plan(M, C, -1, true);
    ln_check_vec(gamma, C, "lscale_fwd", "gamma");
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto y = ln_empty_like(u);
    LN_LAUNCH(k_lscale_fwd, p, p.grid, stream, ln_cptr(u), ln_cptr(resid),
              gamma.data_ptr<float>(), ln_ptr(y), (int)M, (int)C, p.lpr,
              p.rpg, p.groups);
    return y;
}

// (du, dgamma); the residual's gradient is dy itself, the caller passes it on
std::tuple<at::Tensor, at::Tensor> lscale_bwd(at::Tensor dy, at::Tensor u,
                                              at::Tensor gamma, long blocks) {
    ln_check_act(dy, "lscale_bwd", "dy");
    ln_check_act(u, "lscale_bwd", "u");
    TORCH_CHECK(dy.sizes() == u.sizes(), "lscale_bwd: dy shape differs from u");
    const long C = u.size(1), M = u.numel() / std::max<long>(C, 1);
    const LnPlan p = ln_make_plan(M, C, blocks);
    ln_check_vec(gamma, C, "lscale_bwd", "gamma");
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto fopts = u.options().dtype(at::kFloat);
    auto du = ln_empty_like(u);
    auto slab = at::empty({p.grid, C}, fopts);
    auto dgamma = at::empty({C}, fopts);
    LN_LAUNCH(k_lscale_bwd, p, p.grid, stream, ln_cptr(dy), ln_cptr(u),
              gamma.data_ptr<float>(), ln_ptr(du), slab.data_ptr<float>(),
              (int)M, (int)C, p.lpr, p.rpg, p.groups);
    ln_combine(slab, p.grid, (int)C, dgamma.data_ptr<float>(), stream);
    return {du, dgamma};
}

static long gelu_chunks(const at::Tensor& z, const char* who) {
    TORCH_CHECK(z.is_cuda() && z.scalar_type() == at::kBFloat16, who,
                ": needs a bf16 GPU tensor");
    TORCH_CHECK(z.is_non_overlapping_and_dense() && z.numel() % 8 == 0 &&
                z.numel() >= 8, who,
                ": needs a dense tensor with numel % 8 == 0");
    return z.numel() / 8;
}

at::Tensor gelu_fwd(at::Tensor z) {
    const long n8 = gelu_chunks(z, "gelu_fwd");
    auto a = at::empty_like(z);
    hipLaunchKernelGGL(k_gelu_fwd,
                       dim3(std::min<long>(GELU_GRID,
                                           ceil_div_i(n8, LN_BLOCK))),
                       dim3(LN_BLOCK), 0,
                       at::hip::getCurrentHIPStream().stream(), ln_cptr(z),
                       ln_ptr(a), n8);
    HIP_CHECK_LAST();
    return a;
}

at::Tensor gelu_bwd(at::Tensor dy, at::Tensor z) {
    const long n8 = gelu_chunks(z, "gelu_bwd");
    gelu_chunks(dy, "gelu_bwd");
    TORCH_CHECK(dy.sizes() == z.sizes() && dy.strides() == z.strides(),
                "gelu_bwd: dy must have z's shape and layout");
    auto dz = at::empty_like(z);
    hipLaunchKernelGGL(k_gelu_bwd,
                       dim3(std::min<long>(GELU_GRID,
                                           ceil_div_i(n8, LN_BLOCK))),
                       dim3(LN_BLOCK), 0,
                       at::hip::getCurrentHIPStream().stream(), ln_cptr(dy),
                       ln_cptr(z), ln_ptr(dz), n8);
    HIP_CHECK_LAST();
    return dz;
}
