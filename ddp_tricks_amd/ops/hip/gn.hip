// gn.hip — GroupNorm forward/backward over bf16 channels_last activations
// with the fused ReLU / residual epilogue of the BN kernels.
//
// Statistics are per (image, group): the reduction runs over the H*W rows of
// one image and over a slice of Cg = C/G channels inside each row, and the
// normalisation coefficients are per (n, c).  Nothing of bn.hip's per-channel
// work split fits, so the heavy kernels here share one split of their own:
//
//   * a lane owns one 8-channel chunk (16 B) for the block's life; the 256
//     lanes lie flat over (row walker, chunk): tid = walker * slw + ck with
//     slw = min(C/8, 256) chunks and walkers = 256 / slw (lanes past
//     walkers * slw idle; C > 2048 puts further slices on gridDim.y);
//   * a block handles one strip of rows of ONE image — the grid is
//     (strips, slices, N), so n is block-uniform and every per-(n, c)
//     coefficient is loaded once into registers;
//   * walker w takes rows strip_start + w, + walkers, ...: consecutive
//     walkers read consecutive rows.
//
// The heavy kernels never see G: the per-channel partials go to a
// slab[n][s][2][C], and the tiny combine kernels (a wave per (n, g), double
// arithmetic, fixed order) turn them into per-(n, c) coefficient tables.
// No atomics, no device-dependent grid.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

constexpr int GN_BLOCK = 256;
constexpr int GN_MAX_STRIPS = 64;      // cap of the automatic strip count
constexpr int GN_TARGET_BLOCKS = 2048; // strips aim at this many blocks
constexpr int GN_MIN_ROWS = 4;         // a walker's least share of a strip

struct GnPlan { int slw, walkers, S, slices, strip; };

// The one host decision, a function of the shape alone.  strip = rows per
// strip; S = ceil(rows / strip), so no strip is empty.
static GnPlan gn_make_plan(long N, long C, long H, long W, long strips) {
    TORCH_CHECK(N >= 1 && C >= 8 && C % 8 == 0 && H >= 1 && W >= 1,
                "gn_plan: needs N, H, W >= 1 and C % 8 == 0");
    TORCH_CHECK(H * W < (1l << 31) && N < 65536, "gn_plan: shape too large");
    GnPlan p;
    const long chunks = C / 8;
    const long rows = H * W;
    p.slw = (int)std::min<long>(chunks, GN_BLOCK);
    p.walkers = GN_BLOCK / p.slw;
    p.slices = (int)((chunks + p.slw - 1) / p.slw);
    TORCH_CHECK(p.slices < 65536, "gn_plan: C too large");
    long S;
    if (strips > 0) {
        S = std::min<long>(strips, rows);
    } else {
        S = (GN_TARGET_BLOCKS + N * p.slices - 1) / (N * p.slices);
        S = std::min<long>(S, rows / ((long)p.walkers * GN_MIN_ROWS));
        S = std::max<long>(1, std::min<long>(S, GN_MAX_STRIPS));
    }
    p.strip = (int)((rows + S - 1) / S);
    p.S = (int)((rows + p.strip - 1) / p.strip);
    return p;
}

std::tuple<long, long, long, long> gn_plan(long N, long C, long H, long W,
                                           long strips) {
    GnPlan p = gn_make_plan(N, C, H, W, strips);
    return {p.slw, p.walkers, p.S, p.slices};
}

// A lane's place in the split.  off is the element offset of the lane's chunk
// in row r0 + walker of image blockIdx.z; step the element distance between a
// walker's consecutive rows.
struct GnLane {
    bool live;
    int walker, ck, c0, r, r1;
    long off, step;
};

DEV_INLINE GnLane gn_lane(int C, int rows, int slw, int walkers, int strip) {
    GnLane L;
    L.walker = threadIdx.x / slw;
    L.ck = threadIdx.x - L.walker * slw;
    const int chunk = blockIdx.y * slw + L.ck;
    L.c0 = chunk * 8;
    L.live = L.walker < walkers && L.c0 < C;
    const int r0 = blockIdx.x * strip;
    L.r1 = min(rows, r0 + strip);
    L.r = r0 + L.walker;
    L.off = ((long)blockIdx.z * rows + L.r) * C + L.c0;
    L.step = (long)walkers * C;
    return L;
}

DEV_INLINE s16x8 ld8(const bf16* p) {
    return *reinterpret_cast<const s16x8*>(p);
}
DEV_INLINE void st8(bf16* p, s16x8 v) {
    *reinterpret_cast<s16x8*>(p) = v;
}

// Walker join: every lane puts its two 8-channel accumulators into LDS, then
// thread t adds the walkers of channel t, t + 256, ... of the slice in walker
// order and writes slab[n][s][0][c] and slab[n][s][1][c].
DEV_INLINE void gn_join(const GnLane& L, const float (&a)[8],
                        const float (&b)[8], int C, int slw, int walkers,
                        float* __restrict__ slab) {
    __shared__ __attribute__((aligned(16))) float red[2][GN_BLOCK * 8];
    if (L.walker < walkers) {
        f32x4* pa = reinterpret_cast<f32x4*>(&red[0][threadIdx.x * 8]);
        f32x4* pb = reinterpret_cast<f32x4*>(&red[1][threadIdx.x * 8]);
        pa[0] = f32x4{a[0], a[1], a[2], a[3]};
        pa[1] = f32x4{a[4], a[5], a[6], a[7]};
        pb[0] = f32x4{b[0], b[1], b[2], b[3]};
        pb[1] = f32x4{b[4], b[5], b[6], b[7]};
    }
    __syncthreads();
    const int wc = slw * 8;                 // channels of a slice
    const int cbase = blockIdx.y * wc;
    float* out = slab
        + ((long)blockIdx.z * gridDim.x + blockIdx.x) * 2 * (long)C;
    for (int t = threadIdx.x; t < wc && cbase + t < C; t += GN_BLOCK) {
        float ta = 0.f, tb = 0.f;
        for (int w = 0; w < walkers; ++w) {
            ta += red[0][w * wc + t];
            tb += red[1][w * wc + t];
        }
        out[cbase + t] = ta;
        out[C + cbase + t] = tb;
    }
}

// ------------------------------------------------------------- forward -----

DEV_INLINE void gn_acc_stats(s16x8 v, float (&sum)[8], float (&sq)[8]) {
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
        float f = us2f((unsigned short)v[j]);
        sum[j] += f;
        sq[j] = fmaf(f, f, sq[j]);
    }
}

// pass 1: slab[n][s][0][c] = sum x, slab[n][s][1][c] = sum x^2 over the strip
__global__ __launch_bounds__(GN_BLOCK)
void k_gn_partial(const bf16* __restrict__ x, int C, int rows, int slw,
                  int walkers, int strip, float* __restrict__ slab) {
    GnLane L = gn_lane(C, rows, slw, walkers, strip);
    float sum[8] = {}, sq[8] = {};
    if (L.live) {
        const bf16* p = x + L.off;
        int r = L.r;
        // 2-deep: both 16 B loads in flight before either is consumed
        for (; r + walkers < L.r1; r += 2 * walkers, p += 2 * L.step) {
            s16x8 v0 = ld8(p);
            s16x8 v1 = ld8(p + L.step);
            gn_acc_stats(v0, sum, sq);
            gn_acc_stats(v1, sum, sq);
        }
        if (r < L.r1) gn_acc_stats(ld8(p), sum, sq);
    }
    gn_join(L, sum, sq, C, slw, walkers, slab);
}

DEV_INLINE double wave_sum_f64(double v) {
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, 64);
    return __shfl(v, 0, 64);
}

// A wave per (n, g): the S * Cg partials of the group are added in double
// (lane l takes channels l, l + 64, ... of every strip in strip order, then
// the shuffle tree), mean / var in double, invstd rounded to fp32 once;
// coef[n][0][c] = gamma * invstd, coef[n][1][c] = beta - mean * scale.
__global__ __launch_bounds__(GN_BLOCK)
void k_gn_combine(const float* __restrict__ slab, int NG, int G, int C,
                  int S, int rows, const float* __restrict__ gamma,
                  const float* __restrict__ beta, double eps,
                  float* __restrict__ mean, float* __restrict__ invstd,
                  float* __restrict__ coef) {
    const int lane = threadIdx.x & 63;
    const int ng = blockIdx.x * (GN_BLOCK / 64) + (threadIdx.x >> 6);
    if (ng >= NG) return;
    const int n = ng / G, g = ng - n * G;
    const int Cg = C / G;
    double a = 0.0, b = 0.0;
    for (int s = 0; s < S; ++s) {
        const float* p = slab + ((long)n * S + s) * 2 * (long)C + g * Cg;
        for (int c = lane; c < Cg; c += 64) {
            a += (double)p[c];
            b += (double)p[C + c];
        }
    }
    a = wave_sum_f64(a);
    b = wave_sum_f64(b);
    const double m = (double)rows * Cg;
    const double mu = a / m;
    const double var = fmax(b / m - mu * mu, 0.0);
    const float is = (float)(1.0 / sqrt(var + eps));
    if (lane == 0) {
        mean[ng] = (float)mu;
        invstd[ng] = is;
    }
    float* co = coef + (long)n * 2 * C;
    for (int c = g * Cg + lane; c < (g + 1) * Cg; c += 64) {
        const double sc = (double)gamma[c] * (double)is;
        co[c] = (float)sc;
        co[C + c] = (float)((double)beta[c] - mu * sc);
    }
}

template <bool RELU, bool RESID, bool MASK>
DEV_INLINE void gn_apply_row(s16x8 v, s16x8 rv, const float (&sc)[8],
                             const float (&sh)[8], bf16* yp,
                             unsigned char* mp) {
    s16x8 o;
    unsigned m = 0;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
        float f = fmaf(us2f((unsigned short)v[j]), sc[j], sh[j]);
        if (RESID) f += us2f((unsigned short)rv[j]);
        if (RELU) {
            if (f > 0.f) m |= 1u << j;
            f = fmaxf(f, 0.f);
        }
        o[j] = (short)f2us(f);
    }
    st8(yp, o);
    if (MASK) *mp = (unsigned char)m;
}

// pass 2: y = relu?(x * scale[n][c] + shift[n][c] (+ resid)); the mask is one
// byte per chunk, bit j = (pre-rounding value of channel j) > 0 — BN's format.
template <bool RELU, bool RESID, bool MASK>
__global__ __launch_bounds__(GN_BLOCK)
void k_gn_apply(const bf16* __restrict__ x, const bf16* __restrict__ resid,
                const float* __restrict__ coef, bf16* __restrict__ y,
                unsigned char* __restrict__ mask, int C, int rows, int slw,
                int walkers, int strip) {
    GnLane L = gn_lane(C, rows, slw, walkers, strip);
    if (!L.live) return;
    float sc[8], sh[8];
    {
        const float* co = coef + (long)blockIdx.z * 2 * C + L.c0;
        f32x4 a0 = reinterpret_cast<const f32x4*>(co)[0];
        f32x4 a1 = reinterpret_cast<const f32x4*>(co)[1];
        f32x4 b0 = reinterpret_cast<const f32x4*>(co + C)[0];
        f32x4 b1 = reinterpret_cast<const f32x4*>(co + C)[1];
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
            sc[j] = a0[j]; sc[4 + j] = a1[j];
            sh[j] = b0[j]; sh[4 + j] = b1[j];
        }
    }
    long o = L.off;
    long mo = MASK ? o >> 3 : 0;          // C % 8 == 0: one byte per chunk
    const long mstep = L.step >> 3;
    int r = L.r;
    for (; r + walkers < L.r1; r += 2 * walkers) {
        const long o1 = o + L.step;
        s16x8 v0 = ld8(x + o);
        s16x8 v1 = ld8(x + o1);
        s16x8 r0 = RESID ? ld8(resid + o) : s16x8{};
        s16x8 r1 = RESID ? ld8(resid + o1) : s16x8{};
        gn_apply_row<RELU, RESID, MASK>(v0, r0, sc, sh, y + o, mask + mo);
        gn_apply_row<RELU, RESID, MASK>(v1, r1, sc, sh, y + o1,
                                        mask + mo + mstep);
        o += 2 * L.step;
        if (MASK) mo += 2 * mstep;
    }
    if (r < L.r1) {
        s16x8 v0 = ld8(x + o);
        s16x8 r0 = RESID ? ld8(resid + o) : s16x8{};
        gn_apply_row<RELU, RESID, MASK>(v0, r0, sc, sh, y + o, mask + mo);
    }
}

// ------------------------------------------------------------ backward -----

template <bool RELU>
DEV_INLINE void gn_acc_bwd(s16x8 vx, s16x8 vg, unsigned m,
                           const float (&mu)[8], const float (&is)[8],
                           float (&a)[8], float (&b)[8]) {
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
        float g = us2f((unsigned short)vg[j]);
        if (RELU) g = (m >> j) & 1u ? g : 0.f;
        float xh = (us2f((unsigned short)vx[j]) - mu[j]) * is[j];
        a[j] += g;
        b[j] = fmaf(g, xh, b[j]);
    }
}

// slab[n][s][0][c] = A = sum dy_eff, slab[n][s][1][c] = B = sum dy_eff * xhat
// with xhat = (x - mean[n, g(c)]) * invstd[n, g(c)]
template <bool RELU>
__global__ __launch_bounds__(GN_BLOCK)
void k_gn_bwd_partial(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                      const unsigned char* __restrict__ mask,
                      const float* __restrict__ mean,
                      const float* __restrict__ invstd, int G, int Cg, int C,
                      int rows, int slw, int walkers, int strip,
                      float* __restrict__ slab) {
    GnLane L = gn_lane(C, rows, slw, walkers, strip);
    float a[8] = {}, b[8] = {};
    if (L.live) {
        float mu[8], is[8];
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ng = blockIdx.z * G + (L.c0 + j) / Cg;
            mu[j] = mean[ng];
            is[j] = invstd[ng];
        }
        long o = L.off;
        long mo = o >> 3;
        const long mstep = L.step >> 3;
        int r = L.r;
        for (; r + walkers < L.r1; r += 2 * walkers) {
            const long o1 = o + L.step;
            s16x8 x0 = ld8(x + o);
            s16x8 g0 = ld8(dy + o);
            s16x8 x1 = ld8(x + o1);
            s16x8 g1 = ld8(dy + o1);
            unsigned m0 = RELU ? mask[mo] : 0xffu;
            unsigned m1 = RELU ? mask[mo + mstep] : 0xffu;
            gn_acc_bwd<RELU>(x0, g0, m0, mu, is, a, b);
            gn_acc_bwd<RELU>(x1, g1, m1, mu, is, a, b);
            o += 2 * L.step;
            mo += 2 * mstep;
        }
        if (r < L.r1) {
            unsigned m0 = RELU ? mask[mo] : 0xffu;
            gn_acc_bwd<RELU>(ld8(x + o), ld8(dy + o), m0, mu, is, a, b);
        }
    }
    gn_join(L, a, b, C, slw, walkers, slab);
}

// A wave per (n, g), in double: s1 = sum_{c in g} gamma_c A[n,c],
// s2 = sum_{c in g} gamma_c B[n,c], m = rows * Cg; then the coefficients of
// dx = k1 dy_eff + k2 x + k3 for every channel of the group:
//   coef[n][0][c] = k1 = gamma_c invstd
//   coef[n][1][c] = k2 = -invstd^2 s2 / m
//   coef[n][2][c] = k3 = -invstd s1 / m + invstd^2 mean s2 / m
__global__ __launch_bounds__(GN_BLOCK)
void k_gn_bwd_coef(const float* __restrict__ slab, int NG, int G, int C,
                   int S, int rows, const float* __restrict__ gamma,
                   const float* __restrict__ mean,
                   const float* __restrict__ invstd,
                   float* __restrict__ coef) {
    const int lane = threadIdx.x & 63;
    const int ng = blockIdx.x * (GN_BLOCK / 64) + (threadIdx.x >> 6);
    if (ng >= NG) return;
    const int n = ng / G, g = ng - n * G;
    const int Cg = C / G;
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < S; ++s) {
        const float* p = slab + ((long)n * S + s) * 2 * (long)C + g * Cg;
        for (int c = lane; c < Cg; c += 64) {
            const double gm = (double)gamma[g * Cg + c];
            s1 += gm * (double)p[c];
            s2 += gm * (double)p[C + c];
        }
    }
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    const double m = (double)rows * Cg;
    const double mu = (double)mean[ng];
    const double is = (double)invstd[ng];
    const float k2 = (float)(-is * is * s2 / m);
    const float k3 = (float)(-is * s1 / m + is * is * mu * s2 / m);
    float* co = coef + (long)n * 3 * C;
    for (int c = g * Cg + lane; c < (g + 1) * Cg; c += 64) {
        co[c] = (float)((double)gamma[c] * is);
        co[C + c] = k2;
        co[2 * C + c] = k3;
    }
}

// dbeta_c = sum_n sum_s A, dgamma_c = sum_n sum_s B.  A block takes 16
// channels; its 16 x 16 threads lie over (q, channel), thread q adds the
// (n, s) entries q, q + 16, ... in double, the 16 q meet in LDS and are
// added in q order; fp32 out.
constexpr int GN_PQ = 16;
__global__ __launch_bounds__(GN_BLOCK)
void k_gn_bwd_param(const float* __restrict__ slab, int NS, int C,
                    float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double red[2][GN_PQ][GN_PQ];
    const int cl = threadIdx.x & (GN_PQ - 1);
    const int q = threadIdx.x / GN_PQ;
    const int c = blockIdx.x * GN_PQ + cl;
    double a = 0.0, b = 0.0;
    if (c < C) {
        for (int i = q; i < NS; i += GN_PQ) {
            const float* p = slab + (long)i * 2 * C;
            a += (double)p[c];
            b += (double)p[C + c];
        }
    }
    red[0][q][cl] = a;
    red[1][q][cl] = b;
    __syncthreads();
    if (q == 0 && c < C) {
        double ta = 0.0, tb = 0.0;
        #pragma unroll
        for (int w = 0; w < GN_PQ; ++w) {
            ta += red[0][w][cl];
            tb += red[1][w][cl];
        }
        dbeta[c] = (float)ta;
        dgamma[c] = (float)tb;
    }
}

template <bool RELU, bool RESID>
DEV_INLINE void gn_dx_row(s16x8 vx, s16x8 vg, unsigned m,
                          const float (&k1)[8], const float (&k2)[8],
                          const float (&k3)[8], bf16* dxp, bf16* drp) {
    s16x8 o, og;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
        float g = us2f((unsigned short)vg[j]);
        if (RELU) g = (m >> j) & 1u ? g : 0.f;
        float t = fmaf(k2[j], us2f((unsigned short)vx[j]), k3[j]);
        o[j] = (short)f2us(fmaf(k1[j], g, t));
        if (RESID) og[j] = (short)f2us(g);
    }
    st8(dxp, o);
    if (RESID) st8(drp, og);
}

// dx = k1[n][c] dy_eff + k2[n][c] x + k3[n][c]; with a residual the same pass
// writes dresid = dy_eff
template <bool RELU, bool RESID>
__global__ __launch_bounds__(GN_BLOCK)
void k_gn_bwd_dx(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                 const unsigned char* __restrict__ mask,
                 const float* __restrict__ coef, bf16* __restrict__ dx,
                 bf16* __restrict__ dresid, int C, int rows, int slw,
                 int walkers, int strip) {
    GnLane L = gn_lane(C, rows, slw, walkers, strip);
    if (!L.live) return;
    float k1[8], k2[8], k3[8];
    {
        const float* co = coef + (long)blockIdx.z * 3 * C + L.c0;
        #pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 a = reinterpret_cast<const f32x4*>(co)[h];
            f32x4 b = reinterpret_cast<const f32x4*>(co + C)[h];
            f32x4 c = reinterpret_cast<const f32x4*>(co + 2 * C)[h];
            #pragma unroll
            for (int j = 0; j < 4; ++j) {
                k1[4 * h + j] = a[j];
                k2[4 * h + j] = b[j];
                k3[4 * h + j] = c[j];
            }
        }
    }
    long o = L.off;
    long mo = o >> 3;
    const long mstep = L.step >> 3;
    int r = L.r;
    for (; r + walkers < L.r1; r += 2 * walkers) {
        const long o1 = o + L.step;
        s16x8 x0 = ld8(x + o);
        s16x8 g0 = ld8(dy + o);
        s16x8 x1 = ld8(x + o1);
        s16x8 g1 = ld8(dy + o1);
        unsigned m0 = RELU ? mask[mo] : 0xffu;
        unsigned m1 = RELU ? mask[mo + mstep] : 0xffu;
        gn_dx_row<RELU, RESID>(x0, g0, m0, k1, k2, k3, dx + o, dresid + o);
        gn_dx_row<RELU, RESID>(x1, g1, m1, k1, k2, k3, dx + o1, dresid + o1);
        o += 2 * L.step;
        mo += 2 * mstep;
    }
    if (r < L.r1) {
        unsigned m0 = RELU ? mask[mo] : 0xffu;
        gn_dx_row<RELU, RESID>(ld8(x + o), ld8(dy + o), m0, k1, k2, k3,
                               dx + o, dresid + o);
    }
}

// --------------------------------------------------------------- hosts -----

static void gn_check_act(const at::Tensor& t, const char* who,
                         const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                t.dim() == 4, who, ": ", what, " must be bf16 [N,C,H,W]");
    TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast),
                who, ": ", what, " must be channels_last");
}

static void gn_check_vec(const at::Tensor& t, long n, const char* who,
                         const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
                t.is_contiguous() && t.numel() == n,
                who, ": ", what, " must be contiguous fp32 with ", n,
                " elements");
}

static void gn_check_groups(long C, long G, const char* who) {
    TORCH_CHECK(C % 8 == 0, who, ": the HIP path needs C % 8 == 0");
    TORCH_CHECK(G >= 1 && C % G == 0, who, ": num_groups ", G,
                " does not divide C = ", C);
}

static at::Tensor gn_empty_like(const at::Tensor& x) {
    return at::empty_like(
        x, x.options().memory_format(at::MemoryFormat::ChannelsLast));
}

template <bool RELU, bool RESID, bool MASK>
static void gn_launch_apply(const GnPlan& p, dim3 grid, hipStream_t st,
                            const bf16* x, const bf16* r, const float* coef,
                            bf16* y, unsigned char* mask, int C, int rows) {
    hipLaunchKernelGGL((k_gn_apply<RELU, RESID, MASK>), grid, dim3(GN_BLOCK),
                       0, st, x, r, coef, y, mask, C, rows, p.slw, p.walkers,
                       p.strip);
}

// (y, mean[N,G], invstd[N,G], mask); the mask ([N*H*W, C/8] bytes) is written
// only with fuse_relu and want_mask, else it is empty
std::vector<at::Tensor> gn_fwd(at::Tensor x, at::Tensor gamma, at::Tensor beta,
                               long G, double eps, bool fuse_relu,
                               c10::optional<at::Tensor> residual,
                               bool want_mask, long strips) {
    gn_check_act(x, "gn_fwd", "x");
    const long N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
    gn_check_groups(C, G, "gn_fwd");
    gn_check_vec(gamma, C, "gn_fwd", "gamma");
    gn_check_vec(beta, C, "gn_fwd", "beta");
    if (residual.has_value()) {
        gn_check_act(*residual, "gn_fwd", "residual");
        TORCH_CHECK(residual->sizes() == x.sizes(),
                    "gn_fwd: residual shape differs from x");
    }
    const GnPlan p = gn_make_plan(N, C, H, W, strips);
    const int rows = (int)(H * W);
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto fopts = x.options().dtype(at::kFloat);
    auto slab = at::empty({N, p.S, 2, C}, fopts);
    auto mean = at::empty({N, G}, fopts);
    auto invstd = at::empty({N, G}, fopts);
    auto coef = at::empty({N, 2, C}, fopts);
    auto y = gn_empty_like(x);
    const bool mk = fuse_relu && want_mask;
    auto mask = at::empty({mk ? N * rows : 0, mk ? C / 8 : 0},
                          x.options().dtype(at::kByte));
    const bf16* xp = reinterpret_cast<const bf16*>(x.data_ptr());
    const bf16* rp = residual.has_value()
        ? reinterpret_cast<const bf16*>(residual->data_ptr()) : nullptr;
    bf16* yp = reinterpret_cast<bf16*>(y.data_ptr());
    unsigned char* mp = mk ? mask.data_ptr<unsigned char>() : nullptr;
    const dim3 grid(p.S, p.slices, N);

    hipLaunchKernelGGL(k_gn_partial, grid, dim3(GN_BLOCK), 0, stream, xp,
                       (int)C, rows, p.slw, p.walkers, p.strip,
                       slab.data_ptr<float>());
    HIP_CHECK_LAST();
    const int NG = (int)(N * G);
    hipLaunchKernelGGL(k_gn_combine, dim3(ceil_div_i(NG, GN_BLOCK / 64)),
                       dim3(GN_BLOCK), 0, stream, slab.data_ptr<float>(), NG,
                       (int)G, (int)C, p.S, rows, gamma.data_ptr<float>(),
                       beta.data_ptr<float>(), eps, mean.data_ptr<float>(),
                       invstd.data_ptr<float>(), coef.data_ptr<float>());
    HIP_CHECK_LAST();
    const float* cp = coef.data_ptr<float>();
    const int Ci = (int)C;
    if (!fuse_relu) {
        if (rp) gn_launch_apply<false, true, false>(p, grid, stream, xp, rp,
                                                    cp, yp, mp, Ci, rows);
        else gn_launch_apply<false, false, false>(p, grid, stream, xp, rp, cp,
                                                  yp, mp, Ci, rows);
    } else if (mk) {
        if (rp) gn_launch_apply<true, true, true>(p, grid, stream, xp, rp, cp,
                                                  yp, mp, Ci, rows);
        else gn_launch_apply<true, false, true>(p, grid, stream, xp, rp, cp,
                                                yp, mp, Ci, rows);
    } else {
        if (rp) gn_launch_apply<true, true, false>(p, grid, stream, xp, rp,
                                                   cp, yp, mp, Ci, rows);
        else gn_launch_apply<true, false, false>(p, grid, stream, xp, rp, cp,
                                                 yp, mp, Ci, rows);
    }
    HIP_CHECK_LAST();
    return {y, mean, invstd, mask};
}

template <bool RELU>
static void gn_launch_bwd(const GnPlan& p, dim3 grid, hipStream_t st,
                          const bf16* x, const bf16* dy,
                          const unsigned char* mask, const float* mean,
                          const float* invstd, const float* gamma, int N,
                          int G, int C, int rows, float* slab, float* coef,
                          float* dgamma, float* dbeta, bf16* dx,
                          bf16* dresid) {
    hipLaunchKernelGGL(k_gn_bwd_partial<RELU>, grid, dim3(GN_BLOCK), 0, st, x,
                       dy, mask, mean, invstd, G, C / G, C, rows, p.slw,
                       p.walkers, p.strip, slab);
    HIP_CHECK_LAST();
    const int NG = N * G;
    hipLaunchKernelGGL(k_gn_bwd_coef, dim3(ceil_div_i(NG, GN_BLOCK / 64)),
                       dim3(GN_BLOCK), 0, st, slab, NG, G, C, p.S, rows, gamma,
                       mean, invstd, coef);
    HIP_CHECK_LAST();
    hipLaunchKernelGGL(k_gn_bwd_param, dim3(ceil_div_i(C, GN_PQ)),
                       dim3(GN_BLOCK), 0, st, slab, N * p.S, C, dgamma, dbeta);
    HIP_CHECK_LAST();
    if (dresid)
        hipLaunchKernelGGL((k_gn_bwd_dx<RELU, true>), grid, dim3(GN_BLOCK), 0,
                           st, x, dy, mask, coef, dx, dresid, C, rows, p.slw,
                           p.walkers, p.strip);
    else
        hipLaunchKernelGGL((k_gn_bwd_dx<RELU, false>), grid, dim3(GN_BLOCK),
                           0, st, x, dy, mask, coef, dx, dresid, C, rows,
                           p.slw, p.walkers, p.strip);
    HIP_CHECK_LAST();
}

// (dx, dgamma, dbeta[, dresid]); x is the forward's input, mask its mask
std::vector<at::Tensor> gn_bwd(at::Tensor x, at::Tensor dy, at::Tensor gamma,
                               at::Tensor mean, at::Tensor invstd,
                               at::Tensor mask, long G, bool fuse_relu,
                               bool has_residual, long strips) {
    gn_check_act(x, "gn_bwd", "x");
    gn_check_act(dy, "gn_bwd", "dy");
    TORCH_CHECK(dy.sizes() == x.sizes(), "gn_bwd: dy shape differs from x");
    const long N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
    gn_check_groups(C, G, "gn_bwd");
    gn_check_vec(gamma, C, "gn_bwd", "gamma");
    gn_check_vec(mean, N * G, "gn_bwd", "mean");
    gn_check_vec(invstd, N * G, "gn_bwd", "invstd");
    const int rows = (int)(H * W);
    TORCH_CHECK(!fuse_relu ||
                (mask.is_cuda() && mask.scalar_type() == at::kByte &&
                 mask.is_contiguous() && mask.numel() == N * rows * (C / 8)),
                "gn_bwd needs the packed relu mask from gn_fwd");
    const GnPlan p = gn_make_plan(N, C, H, W, strips);
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto fopts = x.options().dtype(at::kFloat);
    auto slab = at::empty({N, p.S, 2, C}, fopts);
    auto coef = at::empty({N, 3, C}, fopts);
    auto dgamma = at::empty({C}, fopts);
    auto dbeta = at::empty({C}, fopts);
    auto dx = gn_empty_like(x);
    at::Tensor dresid;
    bf16* drp = nullptr;
    if (has_residual) {
        dresid = gn_empty_like(x);
        drp = reinterpret_cast<bf16*>(dresid.data_ptr());
    }
    const bf16* xp = reinterpret_cast<const bf16*>(x.data_ptr());
    const bf16* dyp = reinterpret_cast<const bf16*>(dy.data_ptr());
    const unsigned char* mp = fuse_relu
        ? mask.data_ptr<unsigned char>() : nullptr;
    const dim3 grid(p.S, p.slices, N);
    auto run = fuse_relu ? gn_launch_bwd<true> : gn_launch_bwd<false>;
    run(p, grid, stream, xp, dyp, mp, mean.data_ptr<float>(),
        invstd.data_ptr<float>(), gamma.data_ptr<float>(), (int)N, (int)G,
        (int)C, rows, slab.data_ptr<float>(), coef.data_ptr<float>(),
        dgamma.data_ptr<float>(), dbeta.data_ptr<float>(),
        reinterpret_cast<bf16*>(dx.data_ptr()), drp);
    if (has_residual) return {dx, dgamma, dbeta, dresid};
    return {dx, dgamma, dbeta};
}
