// se.hip — Squeeze-and-Excitation junction over bf16 channels_last
// activations:
//
//   y = relu?(u * s[n, c] (+ resid)),  s = sigmoid(a),  a = W2 relu(W1 z + b1) + b2,
//   z[n, c] = mean_hw u
//
// The two tiny FCs between z and a stay on the linear kernels (gemm.hip);
// this file holds the four memory-bound passes around them: the squeeze, the
// gated epilogue, and the backward's two passes over (dy, u).
//
// Work split (the one gn.hip uses, written out here for SE):
//
//   * a lane owns one 8-channel chunk (16 B) for the block's life; the 256
//     lanes lie flat over (row walker, chunk): tid = walker * slw + ck with
//     slw = min(C/8, 256) chunks and walkers = 256 / slw (lanes past
//     walkers * slw idle; C > 2048 puts further slices on gridDim.y);
//   * a block is one strip of rows of ONE image — the grid is
//     (strips, slices, N) — so the lane's 8 gate values s[n][c0..c0+8] and
//     its 8 squeeze-gradient terms dz[n][c] / HW are loaded once and live in
//     registers while the lane walks its rows;
//   * walker w takes rows strip_start + w, + walkers, ...
//
// Per-(n, c) sums (the squeeze, and sum_hw g * u of the gate gradient) go
// walker -> LDS -> slab[n][s][C] -> a thread per (n, c) adding strips in
// order.  With one strip the squeeze block finishes z itself.  No atomics,
// no grid that depends on the device.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

constexpr int SE_BLOCK = 256;
constexpr int SE_MAX_STRIPS = 64;      // cap of the automatic strip count
constexpr int SE_TARGET_BLOCKS = 2048; // strips aim at this many blocks
constexpr int SE_MIN_ROWS = 4;         // a walker's least share of a strip

struct SePlan { int slw, walkers, S, slices, strip; };

// The one host decision, a function of the shape alone.  strip = rows per
// strip; S = ceil(rows / strip), so no strip is empty.
static SePlan se_make_plan(long N, long C, long H, long W, long strips) {
    TORCH_CHECK(N >= 1 && C >= 8 && C % 8 == 0 && H >= 1 && W >= 1,
                "se_plan: needs N, H, W >= 1 and C % 8 == 0");
    TORCH_CHECK(H * W < (1l << 31) && N < 65536, "se_plan: shape too large");
    SePlan p;
    const long chunks = C / 8;
    const long rows = H * W;
    p.slw = (int)std::min<long>(chunks, SE_BLOCK);
    p.walkers = SE_BLOCK / p.slw;
    p.slices = (int)((chunks + p.slw - 1) / p.slw);
    TORCH_CHECK(p.slices < 65536, "se_plan: C too large");
    long S;
    if (strips > 0) {
        S = std::min<long>(strips, rows);
    } else {
        S = (SE_TARGET_BLOCKS + N * p.slices - 1) / (N * p.slices);
        S = std::min<long>(S, rows / ((long)p.walkers * SE_MIN_ROWS));
        S = std::max<long>(1, std::min<long>(S, SE_MAX_STRIPS));
    }
    p.strip = (int)((rows + S - 1) / S);
    p.S = (int)((rows + p.strip - 1) / p.strip);
    return p;
}

std::tuple<long, long, long, long> se_plan(long N, long C, long H, long W,
                                           long strips) {
    SePlan p = se_make_plan(N, C, H, W, strips);
    return {p.slw, p.walkers, p.S, p.slices};
}

// A lane's place in the split.  off is the element offset of the lane's chunk
// in its first row of image blockIdx.z; step the element distance between a
// walker's consecutive rows.  Only a live lane may touch memory at off.
struct SeLane {
    bool live;
    int walker, c0, r, r1;
    long off, step;
};

DEV_INLINE SeLane se_lane(int C, int rows, int slw, int walkers, int strip) {
    SeLane L;
    L.walker = threadIdx.x / slw;
    L.c0 = (blockIdx.y * slw + (threadIdx.x - L.walker * slw)) * 8;
    L.live = L.walker < walkers && L.c0 < C;
    const int r0 = blockIdx.x * strip;
    L.r1 = min(rows, r0 + strip);
    L.r = r0 + L.walker;
    L.off = ((long)blockIdx.z * rows + L.r) * C + L.c0;
    L.step = (long)walkers * C;
    return L;
}

DEV_INLINE s16x8 se_ld8(const bf16* p) {
    return *reinterpret_cast<const s16x8*>(p);
}
DEV_INLINE void se_st8(bf16* p, s16x8 v) {
    *reinterpret_cast<s16x8*>(p) = v;
}

// The gate, one expression for the forward and both backward kernels: a = 0
// gives exactly 0.5; a -> -inf gives 1 / inf = 0, a -> +inf gives 1.
DEV_INLINE float se_sigmoid(float a) {
    return 1.f / (1.f + __expf(-a));
}

// s[j] = sigmoid(a[n][c0 + j]) from the lane's 16 B of bf16 logits
DEV_INLINE void se_load_gate(const bf16* __restrict__ a, int C, int c0,
                             float (&s)[8]) {
    const s16x8 v = se_ld8(a + (long)blockIdx.z * C + c0);
    #pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = se_sigmoid(us2f((unsigned short)v[j]));
}

// Walker join: every lane of a live walker puts its 8 accumulators into LDS
// (dead chunks of the last slice hold zeros); thread t then adds the walkers
// of channel t, t + 256, ... of the slice in walker order.  Returns through
// `emit(c, total)` for every channel c < C of the slice.
template <typename Emit>
DEV_INLINE void se_join(const SeLane& L, const float (&acc)[8], int C,
                        int slw, int walkers, Emit emit) {
    __shared__ __attribute__((aligned(16))) float red[SE_BLOCK * 8];
    if (L.walker < walkers) {
        f32x4* p = reinterpret_cast<f32x4*>(&red[threadIdx.x * 8]);
        p[0] = f32x4{acc[0], acc[1], acc[2], acc[3]};
        p[1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
    }
    __syncthreads();
    const int wc = slw * 8;                 // channels of a slice
    const int cbase = blockIdx.y * wc;
    for (int t = threadIdx.x; t < wc && cbase + t < C; t += SE_BLOCK) {
        float tot = 0.f;
        for (int w = 0; w < walkers; ++w) tot += red[w * wc + t];
        emit(cbase + t, tot);
    }
}

// ------------------------------------------------------------- squeeze -----

DEV_INLINE void se_acc_sum(s16x8 v, float (&sum)[8]) {
    #pragma unroll
    for (int j = 0; j < 8; ++j) sum[j] += us2f((unsigned short)v[j]);
}

// slab[n][s][c] = sum of u over the strip's rows; with one strip (z != null)
// the block writes z[n][c] = bf16(sum / HW) itself and no slab exists.
__global__ __launch_bounds__(SE_BLOCK)
void k_se_squeeze(const bf16* __restrict__ u, int C, int rows, int slw,
                  int walkers, int strip, float* __restrict__ slab,
                  bf16* __restrict__ z) {
    SeLane L = se_lane(C, rows, slw, walkers, strip);
    float sum[8] = {};
    if (L.live) {
        const bf16* p = u + L.off;
        int r = L.r;
        // 4-deep: the loads of four rows are in flight before the first add
        for (; r + 3 * walkers < L.r1; r += 4 * walkers, p += 4 * L.step) {
            s16x8 v0 = se_ld8(p);
            s16x8 v1 = se_ld8(p + L.step);
            s16x8 v2 = se_ld8(p + 2 * L.step);
            s16x8 v3 = se_ld8(p + 3 * L.step);
            se_acc_sum(v0, sum);
            se_acc_sum(v1, sum);
            se_acc_sum(v2, sum);
            se_acc_sum(v3, sum);
        }
        for (; r < L.r1; r += walkers, p += L.step) se_acc_sum(se_ld8(p), sum);
    }
    const long out = z != nullptr
        ? (long)blockIdx.z * C
        : ((long)blockIdx.z * gridDim.x + blockIdx.x) * (long)C;
    const float hw = (float)rows;
    se_join(L, sum, C, slw, walkers, [&](int c, float t) {
        if (z != nullptr)
            reinterpret_cast<unsigned short*>(z)[out + c] = f2us(t / hw);
        else
            slab[out + c] = t;
    });
}

// S > 1: a thread per (n, c) adds the strips in order, divides, rounds once
__global__ __launch_bounds__(SE_BLOCK)
void k_se_squeeze_combine(const float* __restrict__ slab, long NC, int C,
                          int S, int rows, bf16* __restrict__ z) {
    const long i = (long)blockIdx.x * SE_BLOCK + threadIdx.x;
    if (i >= NC) return;
    const long n = i / C;
    const int c = (int)(i - n * C);
    const float* p = slab + n * S * (long)C + c;
    float t = 0.f;
    for (int s = 0; s < S; ++s) t += p[(long)s * C];
    reinterpret_cast<unsigned short*>(z)[i] = f2us(t / (float)rows);
}

// --------------------------------------------------------------- apply -----

template <bool RELU, bool RESID, bool MASK>
DEV_INLINE void se_apply_row(s16x8 v, s16x8 rv, const float (&s)[8], bf16* yp,
                             unsigned char* mp) {
    s16x8 o;
    unsigned m = 0;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float r = RESID ? us2f((unsigned short)rv[j]) : 0.f;
        float f = fmaf(us2f((unsigned short)v[j]), s[j], r);
        if (RELU) {
            if (f > 0.f) m |= 1u << j;
            f = fmaxf(f, 0.f);
        }
        o[j] = (short)f2us(f);
    }
    se_st8(yp, o);
    if (MASK) *mp = (unsigned char)m;
}

// y = relu?(u * sigmoid(a[n][c]) (+ resid)); the mask is one byte per chunk,
// bit j = (pre-rounding value of channel j) > 0 — the BN / GN format.
template <bool RELU, bool RESID, bool MASK>
__global__ __launch_bounds__(SE_BLOCK)
void k_se_apply(const bf16* __restrict__ u, const bf16* __restrict__ resid,
                const bf16* __restrict__ a, bf16* __restrict__ y,
                unsigned char* __restrict__ mask, int C, int rows, int slw,
                int walkers, int strip) {
    SeLane L = se_lane(C, rows, slw, walkers, strip);
    if (!L.live) return;
    float s[8];
    se_load_gate(a, C, L.c0, s);
    long o = L.off;
    long mo = MASK ? o >> 3 : 0;          // C % 8 == 0: one byte per chunk
    const long mstep = L.step >> 3;
    int r = L.r;
    for (; r + walkers < L.r1; r += 2 * walkers) {
        const long o1 = o + L.step;
        s16x8 v0 = se_ld8(u + o);
        s16x8 v1 = se_ld8(u + o1);
        s16x8 r0 = RESID ? se_ld8(resid + o) : s16x8{};
        s16x8 r1 = RESID ? se_ld8(resid + o1) : s16x8{};
        se_apply_row<RELU, RESID, MASK>(v0, r0, s, y + o, mask + mo);
        se_apply_row<RELU, RESID, MASK>(v1, r1, s, y + o1, mask + mo + mstep);
        o += 2 * L.step;
        if (MASK) mo += 2 * mstep;
    }
    if (r < L.r1) {
        s16x8 v0 = se_ld8(u + o);
        s16x8 r0 = RESID ? se_ld8(resid + o) : s16x8{};
        se_apply_row<RELU, RESID, MASK>(v0, r0, s, y + o, mask + mo);
    }
}

// ------------------------------------------------------------ backward -----

template <bool RELU>
DEV_INLINE void se_acc_gu(s16x8 vu, s16x8 vg, unsigned m, float (&t)[8]) {
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
        float g = us2f((unsigned short)vg[j]);
        if (RELU) g = (m >> j) & 1u ? g : 0.f;
        t[j] = fmaf(g, us2f((unsigned short)vu[j]), t[j]);
    }
}

// slab[n][s][c] = sum over the strip of g * u, g = dy where the mask bit is
// set (all of dy without RELU)
template <bool RELU>
__global__ __launch_bounds__(SE_BLOCK)
void k_se_bwd_partial(const bf16* __restrict__ u, const bf16* __restrict__ dy,
                      const unsigned char* __restrict__ mask, int C, int rows,
                      int slw, int walkers, int strip,
                      float* __restrict__ slab) {
    SeLane L = se_lane(C, rows, slw, walkers, strip);
    float t[8] = {};
    if (L.live) {
        long o = L.off;
        long mo = o >> 3;
        const long mstep = L.step >> 3;
        int r = L.r;
        for (; r + walkers < L.r1; r += 2 * walkers) {
            const long o1 = o + L.step;
            s16x8 u0 = se_ld8(u + o);
            s16x8 g0 = se_ld8(dy + o);
            s16x8 u1 = se_ld8(u + o1);
            s16x8 g1 = se_ld8(dy + o1);
            unsigned m0 = RELU ? mask[mo] : 0xffu;
            unsigned m1 = RELU ? mask[mo + mstep] : 0xffu;
            se_acc_gu<RELU>(u0, g0, m0, t);
            se_acc_gu<RELU>(u1, g1, m1, t);
            o += 2 * L.step;
            mo += 2 * mstep;
        }
        if (r < L.r1) {
            unsigned m0 = RELU ? mask[mo] : 0xffu;
            se_acc_gu<RELU>(se_ld8(u + o), se_ld8(dy + o), m0, t);
        }
    }
    float* so = slab + ((long)blockIdx.z * gridDim.x + blockIdx.x) * (long)C;
    se_join(L, t, C, slw, walkers, [&](int c, float v) { so[c] = v; });
}

// A thread per (n, c): t = strips in order, da = bf16(t * s * (1 - s)) with
// s recomputed from the logit by the apply's expression
__global__ __launch_bounds__(SE_BLOCK)
void k_se_bwd_gate(const float* __restrict__ slab, const bf16* __restrict__ a,
                   long NC, int C, int S, bf16* __restrict__ da) {
    const long i = (long)blockIdx.x * SE_BLOCK + threadIdx.x;
    if (i >= NC) return;
    const long n = i / C;
    const int c = (int)(i - n * C);
    const float* p = slab + n * S * (long)C + c;
    float t = 0.f;
    for (int s = 0; s < S; ++s) t += p[(long)s * C];
    const float s = se_sigmoid(bf2f(a[i]));
    reinterpret_cast<unsigned short*>(da)[i] = f2us(t * s * (1.f - s));
}

template <bool RELU, bool RESID>
DEV_INLINE void se_dx_row(s16x8 vg, unsigned m, const float (&s)[8],
                          const float (&q)[8], bf16* dxp, bf16* drp) {
    s16x8 o, og;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
        float g = us2f((unsigned short)vg[j]);
        if (RELU) g = (m >> j) & 1u ? g : 0.f;
        o[j] = (short)f2us(fmaf(g, s[j], q[j]));
        if (RESID) og[j] = (short)f2us(g);
    }
    se_st8(dxp, o);
    if (RESID) se_st8(drp, og);
}

// dx = g * s[n][c] + dz[n][c] / HW: the gate path's gradient through the
// squeeze enters here and is never a tensor.  RESID (only with RELU: without
// it dresid is dy itself) writes dresid = g in the same pass.  u is not read.
template <bool RELU, bool RESID>
__global__ __launch_bounds__(SE_BLOCK)
void k_se_bwd_dx(const bf16* __restrict__ dy,
                 const unsigned char* __restrict__ mask,
                 const bf16* __restrict__ a, const bf16* __restrict__ dz,
                 bf16* __restrict__ dx, bf16* __restrict__ dresid, int C,
                 int rows, int slw, int walkers, int strip) {
    static_assert(RELU || !RESID, "without relu dresid is dy");
    SeLane L = se_lane(C, rows, slw, walkers, strip);
    if (!L.live) return;
    float s[8], q[8];
    se_load_gate(a, C, L.c0, s);
    {
        const s16x8 v = se_ld8(dz + (long)blockIdx.z * C + L.c0);
        const float hw = (float)rows;
        #pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = us2f((unsigned short)v[j]) / hw;
    }
    long o = L.off;
    long mo = o >> 3;
    const long mstep = L.step >> 3;
    int r = L.r;
    for (; r + walkers < L.r1; r += 2 * walkers) {
        const long o1 = o + L.step;
        s16x8 g0 = se_ld8(dy + o);
        s16x8 g1 = se_ld8(dy + o1);
        unsigned m0 = RELU ? mask[mo] : 0xffu;
        unsigned m1 = RELU ? mask[mo + mstep] : 0xffu;
        se_dx_row<RELU, RESID>(g0, m0, s, q, dx + o, dresid + o);
        se_dx_row<RELU, RESID>(g1, m1, s, q, dx + o1, dresid + o1);
        o += 2 * L.step;
        mo += 2 * mstep;
    }
    if (r < L.r1) {
        unsigned m0 = RELU ? mask[mo] : 0xffu;
        se_dx_row<RELU, RESID>(se_ld8(dy + o), m0, s, q, dx + o, dresid + o);
    }
}

// --------------------------------------------------------------- hosts -----

static void se_check_act(const at::Tensor& t, const char* who,
                         const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                t.dim() == 4, who, ": ", what, " must be bf16 [N,C,H,W]");
    TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast),
                who, ": ", what, " must be channels_last");
    TORCH_CHECK(((uintptr_t)t.data_ptr() & 15) == 0, who, ": ", what,
                " must be 16-byte aligned");
}

// a per-(n, c) bf16 operand: the gate logits, or dz
static void se_check_nc(const at::Tensor& t, long N, long C, const char* who,
                        const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                t.dim() == 2 && t.size(0) == N && t.size(1) == C &&
                t.is_contiguous(), who, ": ", what,
                " must be contiguous bf16 [", N, ", ", C, "]");
    TORCH_CHECK(((uintptr_t)t.data_ptr() & 15) == 0, who, ": ", what,
                " must be 16-byte aligned");
}

static void se_check_mask(const at::Tensor& mask, long bytes,
                          const char* who) {
    TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == at::kByte &&
                mask.is_contiguous() && mask.numel() == bytes,
                who, " needs the packed relu mask from se_apply");
}

static at::Tensor se_empty_like(const at::Tensor& x) {
    return at::empty_like(
        x, x.options().memory_format(at::MemoryFormat::ChannelsLast));
}

static const bf16* se_cptr(const at::Tensor& t) {
    return reinterpret_cast<const bf16*>(t.data_ptr());
}
static bf16* se_ptr(at::Tensor& t) {
    return reinterpret_cast<bf16*>(t.data_ptr());
}

// z[N, C] bf16 = mean over (H, W) of u: fp32 sums, one true division, one RNE
at::Tensor se_squeeze(at::Tensor u, long strips) {
    se_check_act(u, "se_squeeze", "u");
    const long N = u.size(0), C = u.size(1), H = u.size(2), W = u.size(3);
    TORCH_CHECK(C % 8 == 0, "se_squeeze: the HIP path needs C % 8 == 0");
    const SePlan p = se_make_plan(N, C, H, W, strips);
    const int rows = (int)(H * W);
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto z = at::empty({N, C}, u.options());
    const dim3 grid(p.S, p.slices, N);
    if (p.S == 1) {
        hipLaunchKernelGGL(k_se_squeeze, grid, dim3(SE_BLOCK), 0, stream,
                           se_cptr(u), (int)C, rows, p.slw, p.walkers, p.strip,
                           (float*)nullptr, se_ptr(z));
        HIP_CHECK_LAST();
        return z;
    }
    auto slab = at::empty({N, p.S, C}, z.options().dtype(at::kFloat));
    hipLaunchKernelGGL(k_se_squeeze, grid, dim3(SE_BLOCK), 0, stream,
                       se_cptr(u), (int)C, rows, p.slw, p.walkers, p.strip,
                       slab.data_ptr<float>(), (bf16*)nullptr);
    HIP_CHECK_LAST();
    hipLaunchKernelGGL(k_se_squeeze_combine,
                       dim3(ceil_div_i(N * C, SE_BLOCK)), dim3(SE_BLOCK), 0,
                       stream, slab.data_ptr<float>(), N * C, (int)C, p.S,
                       rows, se_ptr(z));
    HIP_CHECK_LAST();
    return z;
}

template <bool RELU, bool RESID, bool MASK>
static void se_launch_apply(const SePlan& p, dim3 grid, hipStream_t st,
                            const bf16* u, const bf16* r, const bf16* a,
                            bf16* y, unsigned char* mask, int C, int rows) {
    hipLaunchKernelGGL((k_se_apply<RELU, RESID, MASK>), grid, dim3(SE_BLOCK),
                       0, st, u, r, a, y, mask, C, rows, p.slw, p.walkers,
                       p.strip);
}

// (y, mask): y = relu?(u * sigmoid(a)[n, c] (+ residual)): plain scale,
// relu, relu + residual, and the residual without relu; the mask
// ([N*H*W, C/8] bytes) is written only with fuse_relu and want_mask, else it
// is empty.
std::tuple<at::Tensor, at::Tensor> se_apply(
        at::Tensor u, at::Tensor a, c10::optional<at::Tensor> residual,
        bool fuse_relu, bool want_mask) {
    se_check_act(u, "se_apply", "u");
    const long N = u.size(0), C = u.size(1), H = u.size(2), W = u.size(3);
    TORCH_CHECK(C % 8 == 0, "se_apply: the HIP path needs C % 8 == 0");
    se_check_nc(a, N, C, "se_apply", "a");
    if (residual.has_value()) {
        se_check_act(*residual, "se_apply", "residual");
        TORCH_CHECK(residual->sizes() == u.sizes(),
                    "se_apply: residual shape differs from u");
    }
    const SePlan p = se_make_plan(N, C, H, W, -1);
    const int rows = (int)(H * W);
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto y = se_empty_like(u);
    const bool mk = fuse_relu && want_mask;
    auto mask = at::empty({mk ? N * rows : 0, mk ? C / 8 : 0},
                          u.options().dtype(at::kByte));
    const bf16* rp = residual.has_value() ? se_cptr(*residual) : nullptr;
    unsigned char* mp = mk ? mask.data_ptr<unsigned char>() : nullptr;
    const dim3 grid(p.S, p.slices, N);
    const int Ci = (int)C;
    if (!fuse_relu) {
        if (rp) se_launch_apply<false, true, false>(p, grid, stream,
                                                    se_cptr(u), rp, se_cptr(a),
                                                    se_ptr(y), mp, Ci, rows);
        else se_launch_apply<false, false, false>(p, grid, stream, se_cptr(u),
                                                  rp, se_cptr(a), se_ptr(y),
                                                  mp, Ci, rows);
    } else if (mk) {
        if (rp) se_launch_apply<true, true, true>(p, grid, stream, se_cptr(u),
                                                  rp, se_cptr(a), se_ptr(y),
                                                  mp, Ci, rows);
        else se_launch_apply<true, false, true>(p, grid, stream, se_cptr(u),
                                                rp, se_cptr(a), se_ptr(y), mp,
                                                Ci, rows);
    } else {
        if (rp) se_launch_apply<true, true, false>(p, grid, stream, se_cptr(u),
                                                   rp, se_cptr(a), se_ptr(y),
                                                   mp, Ci, rows);
        else se_launch_apply<true, false, false>(p, grid, stream, se_cptr(u),
                                                 rp, se_cptr(a), se_ptr(y), mp,
                                                 Ci, rows);
    }
    HIP_CHECK_LAST();
    return {y, mask};
}

// da[N, C] bf16 = (sum_hw g * u) * s * (1 - s), the gradient at the logits
at::Tensor se_bwd_gate(at::Tensor dy, at::Tensor u, at::Tensor mask,
                       at::Tensor a, bool fuse_relu, long strips) {
    se_check_act(u, "se_bwd_gate", "u");
    se_check_act(dy, "se_bwd_gate", "dy");
    TORCH_CHECK(dy.sizes() == u.sizes(), "se_bwd_gate: dy shape differs from u");
    const long N = u.size(0), C = u.size(1), H = u.size(2), W = u.size(3);
    TORCH_CHECK(C % 8 == 0, "se_bwd_gate: the HIP path needs C % 8 == 0");
    se_check_nc(a, N, C, "se_bwd_gate", "a");
    const int rows = (int)(H * W);
    if (fuse_relu) se_check_mask(mask, N * rows * (C / 8), "se_bwd_gate");
    const SePlan p = se_make_plan(N, C, H, W, strips);
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto slab = at::empty({N, p.S, C}, a.options().dtype(at::kFloat));
    auto da = at::empty_like(a);
    const unsigned char* mp = fuse_relu
        ? mask.data_ptr<unsigned char>() : nullptr;
    const dim3 grid(p.S, p.slices, N);
    if (fuse_relu)
        hipLaunchKernelGGL(k_se_bwd_partial<true>, grid, dim3(SE_BLOCK), 0,
                           stream, se_cptr(u), se_cptr(dy), mp, (int)C, rows,
                           p.slw, p.walkers, p.strip, slab.data_ptr<float>());
    else
        hipLaunchKernelGGL(k_se_bwd_partial<false>, grid, dim3(SE_BLOCK), 0,
                           stream, se_cptr(u), se_cptr(dy), mp, (int)C, rows,
                           p.slw, p.walkers, p.strip, slab.data_ptr<float>());
    HIP_CHECK_LAST();
    hipLaunchKernelGGL(k_se_bwd_gate, dim3(ceil_div_i(N * C, SE_BLOCK)),
                       dim3(SE_BLOCK), 0, stream, slab.data_ptr<float>(),
                       se_cptr(a), N * C, (int)C, p.S, se_ptr(da));
    HIP_CHECK_LAST();
    return da;
}

// (dx, dresid): dx = g * s + dz / HW; dresid = g with a residual (dy itself
// without relu — returned, not copied), None without one.  u is taken for its
// shape and for symmetry with se_bwd_gate; the kernel does not read it.
std::tuple<at::Tensor, c10::optional<at::Tensor>> se_bwd_dx(
        at::Tensor dy, at::Tensor u, at::Tensor mask, at::Tensor a,
        at::Tensor dz, bool fuse_relu, bool has_residual) {
    se_check_act(u, "se_bwd_dx", "u");
    se_check_act(dy, "se_bwd_dx", "dy");
    TORCH_CHECK(dy.sizes() == u.sizes(), "se_bwd_dx: dy shape differs from u");
    const long N = u.size(0), C = u.size(1), H = u.size(2), W = u.size(3);
    TORCH_CHECK(C % 8 == 0, "se_bwd_dx: the HIP path needs C % 8 == 0");
    se_check_nc(a, N, C, "se_bwd_dx", "a");
    se_check_nc(dz, N, C, "se_bwd_dx", "dz");
    const int rows = (int)(H * W);
    if (fuse_relu) se_check_mask(mask, N * rows * (C / 8), "se_bwd_dx");
    const SePlan p = se_make_plan(N, C, H, W, -1);
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto dx = se_empty_like(dy);
    c10::optional<at::Tensor> dresid;
    const unsigned char* mp = fuse_relu
        ? mask.data_ptr<unsigned char>() : nullptr;
    const dim3 grid(p.S, p.slices, N);
    const int Ci = (int)C;
    if (!fuse_relu) {
        if (has_residual) dresid = dy;
        hipLaunchKernelGGL((k_se_bwd_dx<false, false>), grid, dim3(SE_BLOCK),
                           0, stream, se_cptr(dy), mp, se_cptr(a), se_cptr(dz),
                           se_ptr(dx), (bf16*)nullptr, Ci, rows, p.slw,
                           p.walkers, p.strip);
    } else if (has_residual) {
        at::Tensor dr = se_empty_like(dy);
        hipLaunchKernelGGL((k_se_bwd_dx<true, true>), grid, dim3(SE_BLOCK), 0,
                           stream, se_cptr(dy), mp, se_cptr(a), se_cptr(dz),
                           se_ptr(dx), se_ptr(dr), Ci, rows, p.slw, p.walkers,
                           p.strip);
        dresid = dr;
    } else {
        hipLaunchKernelGGL((k_se_bwd_dx<true, false>), grid, dim3(SE_BLOCK),
                           0, stream, se_cptr(dy), mp, se_cptr(a), se_cptr(dz),
                           se_ptr(dx), (bf16*)nullptr, Ci, rows, p.slw,
                           p.walkers, p.strip);
    }
    HIP_CHECK_LAST();
    return {dx, dresid};
}
