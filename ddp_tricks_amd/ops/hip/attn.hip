// attn.hip — non-causal multi-head self-attention with head dimension 64 over
// a packed bf16 channels_last qkv activation, forward and backward, and the
// position-table add of the ViT stem.
//
// Operands.  qkv is [N, 3D, H, W] channels_last, D = 64 heads: a matrix of
// N L rows (L = H W tokens) of 3D bf16, head h's q at columns [64h, 64h + 64),
// its k at D + 64h, its v at 2D + 64h — what a Conv2d(D, 3D, 1) writes.  The
// output o is [N, D, H, W] channels_last with head h at [64h, 64h + 64), lse
// [N, heads, L] fp32 the natural log-sum-exp of the scaled logits.  dqkv has
// qkv's layout; every element of it is written by exactly one block of one
// kernel: no atomics, no zero fill, the same bits at every launch.
//
// One MFMA orientation serves all seven GEMMs.  With X and Y fragments in the
// v_mfma_f32_16x16x32_bf16 operand format (lane (g, lg) = (lane & 15,
// lane >> 4) holds row g, k-slots 8 lg + j), mma(X, Y) leaves in lane (g, lg),
// register r, the entry (X row 4 lg + r, Y row g).  The rows a wave OWNS are
// always the Y operand and stay in registers for the block's life; the rows
// it STREAMS are the X operand, read from LDS.  So after a score GEMM a lane
// holds, for its own row g, four consecutive streamed rows per 16-row
// sub-tile, and
//   * the per-row softmax state (max, sum, lse, delta) of an owned row is a
//     per-lane scalar: the only cross-lane traffic is two xor-shuffles over
//     the four lane groups;
//   * two sub-tiles' registers, rounded to bf16, ARE the Y fragment of the
//     second GEMM, with k-slot 8 lg + j standing for streamed row
//     16 (j / 4) + 4 lg + j % 4 of a 32-row chunk.  P never touches LDS.
//   * The X operand of the second GEMM is the streamed tile transposed
//     (row = channel d, k-slots = streamed rows in that same order):
//     ds_read_tr16_b64 twice, the halves 16 rows apart.
// Forward, per 64-key tile:  S^T = K Q^T (X = K rows, Y = Q), online softmax,
// O^T += V^T P^T (X = V transposed, Y = P).  The issue's sketch had P as the
// A operand (O = P V); the transposed product is the same instruction with
// the operands swapped and leaves the output row in the lane that holds its
// max and sum, which saves the four ds_bpermutes per tile that rescaling an
// O accumulator laid out by rows 4 lg + r would need.
//
// The scale 0.125 is folded with log2 e into one constant: t = s * C2,
// C2 = fl(0.125 log2 e), applied to the fp32 logits as they leave the MFMA;
// max, exp2 and lse work on t.  dq and dk are multiplied by 0.125 (exact) in
// their epilogues.
//
// Staging: 64 x 64 bf16 images (128 B rows) by global_load_lds, 16 B per lane,
// 16 B segment ^ (row & 7) on the source address and again on the reads (the
// image of k_gconv_wgrad).  Rows past L source a zeroed 16 B buffer; no lane
// forms an address outside its tensor.  Two image pairs: tile t + 1 is in
// flight while tile t is multiplied, one barrier per tile.  32 KiB of LDS
// (33 KiB in k_attn_bwd_dkv, which also streams lse and delta, 4 B per lane).
// Epilogues round to bf16 into a dead image and write 16 B chunks, 128 B
// contiguous per row.
//
// Backward recomputes the scores twice rather than add dq with atomics:
//   k_attn_bwd_dq   owns 64 queries (q, do; delta = sum_d do o in its
//                   prologue, written for the second kernel), streams K and V:
//                   S^T, dP^T = V dO^T, dS = P (dP - delta), dQ^T += K^T dS^T.
//   k_attn_bwd_dkv  owns 64 keys (k, v), streams Q and dO with lse and delta:
//                   S = Q K^T, dP = dO V^T, dV^T += dO^T P, dK^T += Q^T dS.
// 3 + 4 = 7 tile GEMMs per tile pair where an atomic-dQ design runs 5.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <string>
#include <tuple>
#include "common.h"

typedef short at_bf16x8 __attribute__((ext_vector_type(8)));
typedef short at_bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) at_bf16x4* at_lds_tr16_ptr;
typedef __attribute__((address_space(3))) unsigned int* at_lds_u32_ptr;
typedef const __attribute__((address_space(1))) unsigned int* at_glb_u32_ptr;

static __device__ __align__(16) unsigned char at_zero16[16];

constexpr int AT_D = 64;             // head dimension
constexpr int AT_T = 64;             // rows of a block's tile and of a streamed tile
constexpr int AT_BLOCK = 256;
constexpr int AT_IMG = AT_T * AT_D;  // elements of one LDS image
constexpr float AT_LOG2E = 1.44269504088896341f;
constexpr float AT_LN2 = 0.693147180559945309f;
constexpr float AT_C2 = 0.125f * AT_LOG2E;
constexpr int AP_GRID = 2048;

DEV_INLINE short at_f2bf_bits(float f) {
    return __builtin_bit_cast(short, (__bf16)f);
}

DEV_INLINE at_bf16x8 at_pack8(f32x4 a, f32x4 b) {
    at_bf16x8 o;
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
        o[r] = at_f2bf_bits(a[r]);
        o[4 + r] = at_f2bf_bits(b[r]);
    }
    return o;
}

// sum / max over the four lane groups of a row: every lane ends with the
// same bits
DEV_INLINE float at_sum4(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}
DEV_INLINE float at_max4(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}

struct AtLane {
    int tid, lane, wid, g, lg;
    unsigned long zaddr;
};

DEV_INLINE AtLane at_lane() {
    AtLane T;
    T.tid = threadIdx.x;
    T.lane = T.tid & 63;
    T.wid = __builtin_amdgcn_readfirstlane(T.tid >> 6);
    T.g = T.lane & 15;
    T.lg = T.lane >> 4;
    T.zaddr = reinterpret_cast<unsigned long>(at_zero16);
    asm volatile("" : "+s"(T.zaddr));
    return T;
}

// rows [row0, row0 + 64) of a matrix with `ld` elements per row, 64 columns
// from src, into img; wave wid fills the 8-row chunks wid and wid + 4
DEV_INLINE void at_stage(const AtLane& T, const bf16* __restrict__ src, int ld,
                         int row0, int L, bf16* img) {
    const int srow = T.lane >> 3;
    const int seg8 = ((T.lane & 7) ^ srow) * 8;
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = row0 + (T.wid + 4 * i) * 8 + srow;
        const unsigned long a = row < L
            ? reinterpret_cast<unsigned long>(src + (long)row * ld + seg8)
            : T.zaddr;
        __builtin_amdgcn_global_load_lds(
            reinterpret_cast<const __attribute__((address_space(1)))
                             unsigned short*>(a),
            (__attribute__((address_space(3))) unsigned short*)(
                img + (T.wid + 4 * i) * 512), 16, 0, 0);
    }
}

// X fragment of the image's rows 16 st + g over columns [32 ks, 32 ks + 32)
DEV_INLINE at_bf16x8 at_frag(const AtLane& T, const bf16* img, int st, int ks) {
    const int row = 16 * st + T.g;
    return *reinterpret_cast<const at_bf16x8*>(
        img + row * AT_D + (((4 * ks + T.lg) ^ (row & 7)) << 3));
}

// X fragment of the transposed image: row = column 16 dt + g, k-slot 8 lg + j
// = image row 32 c + 16 (j / 4) + 4 lg + j % 4
DEV_INLINE at_bf16x8 at_frag_t(const AtLane& T, const bf16* img, int c, int dt) {
    const int row = 32 * c + 4 * T.lg + (T.g >> 2);
    const int seg = 2 * dt + ((T.g & 3) >> 1);
    const bf16* p = img + row * AT_D + ((seg ^ (row & 7)) << 3) + (T.g & 1) * 4;
    const at_bf16x4 lo =
        __builtin_amdgcn_ds_read_tr16_b64_v4i16((at_lds_tr16_ptr)p);
    const at_bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (at_lds_tr16_ptr)(p + 16 * AT_D));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// Y fragments of the wave's own 16 rows, straight from memory
DEV_INLINE void at_own(const AtLane& T, const bf16* __restrict__ src, int ld,
                       int row0, int L, at_bf16x8 (&f)[2]) {
    const int row = row0 + 16 * T.wid + T.g;
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks)
        f[ks] = row < L ? *reinterpret_cast<const at_bf16x8*>(
                              src + (long)row * ld + 32 * ks + 8 * T.lg)
                        : at_bf16x8{};
}

// Block barrier that first lands this wave's in-flight global_load_lds: a
// workgroup-scope release does not wait for vmcnt, and the other waves read
// what this one's DMA writes.
DEV_INLINE void at_barrier() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

DEV_INLINE f32x4 at_mma(at_bf16x8 x, at_bf16x8 y, f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, y, acc, 0, 0, 0);
}

// acc[dt][r] is (own row 16 wid + g, column 16 dt + 4 lg + r): times mul, to
// bf16 through `stage` (a dead image, same swizzle), then rows
// [row0, row0 + 64) below L of dst as 16 B chunks.  The caller has passed a
// barrier since the last read of `stage`.
DEV_INLINE void at_store_tile(const AtLane& T, const f32x4 (&acc)[4], float mul,
                              bf16* stage, bf16* __restrict__ dst, int ld,
                              int row0, int L) {
    const int row = 16 * T.wid + T.g;
    #pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        at_bf16x4 v;
        #pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = at_f2bf_bits(acc[dt][r] * mul);
        const int seg = 2 * dt + (T.lg >> 1);
        *reinterpret_cast<at_bf16x4*>(
            stage + row * AT_D + ((seg ^ (row & 7)) << 3) + (T.lg & 1) * 4) = v;
    }
    __syncthreads();
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int id = T.tid + AT_BLOCK * i;
        const int r = id >> 3, sg = id & 7;
        const s16x8 v = *reinterpret_cast<const s16x8*>(
            stage + r * AT_D + ((sg ^ (r & 7)) << 3));
        if (row0 + r < L)
            *reinterpret_cast<s16x8*>(dst + (long)(row0 + r) * ld + sg * 8) = v;
    }
}

// ---------------------------------------------------------------- forward ---

// grid (ceil(L / 64), heads, N): the block's 64 queries, 16 per wave
template <bool SAVE>
__global__ __launch_bounds__(AT_BLOCK)
void k_attn_fwd(const bf16* __restrict__ qkv, bf16* __restrict__ o,
                float* __restrict__ lse, int L, int heads) {
    __shared__ __align__(16) bf16 img_k0[AT_IMG];
    __shared__ __align__(16) bf16 img_v0[AT_IMG];
    __shared__ __align__(16) bf16 img_k1[AT_IMG];
    __shared__ __align__(16) bf16 img_v1[AT_IMG];
    const AtLane T = at_lane();
    const int D = heads * AT_D, ld = 3 * D;
    const int h = blockIdx.y, n = blockIdx.z, q0 = blockIdx.x * AT_T;
    const bf16* qb = qkv + (long)n * L * ld + h * AT_D;
    const bf16* kb = qb + D;
    const bf16* vb = qb + 2 * D;
    const int nt = (L + AT_T - 1) / AT_T;

    at_bf16x8 qf[2];
    at_own(T, qb, ld, q0, L, qf);

    f32x4 acc[4] = {};
    float m = -INFINITY, l = 0.f;   // l: this lane's keys only, joined at the end
    auto tile = [&](int t, const bf16* ik, const bf16* iv)
                    __attribute__((always_inline)) {
        f32x4 s[4];
        #pragma unroll
        for (int st = 0; st < 4; ++st) {
            s[st] = f32x4{};
            #pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                s[st] = at_mma(at_frag(T, ik, st, ks), qf[ks], s[st]);
        }
        float mx = -INFINITY;
        #pragma unroll
        for (int st = 0; st < 4; ++st)
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = t * AT_T + 16 * st + 4 * T.lg + r;
                s[st][r] = key < L ? s[st][r] * AT_C2 : -INFINITY;
                mx = fmaxf(mx, s[st][r]);
            }
        const float mn = fmaxf(m, at_max4(mx));   // finite: key t * 64 exists
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        float ps = 0.f;
        #pragma unroll
        for (int st = 0; st < 4; ++st)
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[st][r] = __builtin_amdgcn_exp2f(s[st][r] - mn);
                ps += s[st][r];
            }
        l = fmaf(l, alpha, ps);
        #pragma unroll
        for (int dt = 0; dt < 4; ++dt) acc[dt] *= alpha;
        #pragma unroll
        for (int c = 0; c < 2; ++c) {
            const at_bf16x8 pf = at_pack8(s[2 * c], s[2 * c + 1]);
            #pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                acc[dt] = at_mma(at_frag_t(T, iv, c, dt), pf, acc[dt]);
        }
    };
    auto issue = [&](int t, bf16* ik, bf16* iv) __attribute__((always_inline)) {
        at_stage(T, kb, ld, t * AT_T, L, ik);
        at_stage(T, vb, ld, t * AT_T, L, iv);
    };

    issue(0, img_k0, img_v0);
    for (int t = 0; t < nt; t += 2) {
        at_barrier();               // tile t landed; pair 1 is free
        if (t + 1 < nt) issue(t + 1, img_k1, img_v1);
        tile(t, img_k0, img_v0);
        if (t + 1 >= nt) break;
        at_barrier();
        if (t + 2 < nt) issue(t + 2, img_k0, img_v0);
        tile(t + 1, img_k1, img_v1);
    }
    at_barrier();                   // every fragment read retired

    l = at_sum4(l);
    const int row = q0 + 16 * T.wid + T.g;
    if (SAVE && T.lg == 0 && row < L)
        lse[((long)n * heads + h) * L + row] = fmaf(m, AT_LN2, logf(l));
    at_store_tile(T, acc, 1.f / l, img_k0, o + (long)n * L * D + h * AT_D, D,
                  q0, L);
}

// ------------------------------------------------------------ backward dq ---

// grid as the forward's.  delta [N, heads, L] is written here.
__global__ __launch_bounds__(AT_BLOCK)
void k_attn_bwd_dq(const bf16* __restrict__ qkv, const bf16* __restrict__ o,
                   const bf16* __restrict__ dO, const float* __restrict__ lse,
                   float* __restrict__ delta, bf16* __restrict__ dqkv, int L,
                   int heads) {
    __shared__ __align__(16) bf16 img_k0[AT_IMG];
    __shared__ __align__(16) bf16 img_v0[AT_IMG];
    __shared__ __align__(16) bf16 img_k1[AT_IMG];
    __shared__ __align__(16) bf16 img_v1[AT_IMG];
    const AtLane T = at_lane();
    const int D = heads * AT_D, ld = 3 * D;
    const int h = blockIdx.y, n = blockIdx.z, q0 = blockIdx.x * AT_T;
    const long hoff = (long)n * L * ld + h * AT_D;
    const long ooff = (long)n * L * D + h * AT_D;
    const bf16* kb = qkv + hoff + D;
    const bf16* vb = qkv + hoff + 2 * D;
    const int nt = (L + AT_T - 1) / AT_T;

    at_bf16x8 qf[2], dof[2], of[2];
    at_own(T, qkv + hoff, ld, q0, L, qf);
    at_own(T, dO + ooff, D, q0, L, dof);
    at_own(T, o + ooff, D, q0, L, of);
    float dl = 0.f;
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks)
        #pragma unroll
        for (int e = 0; e < 8; ++e)
            dl = fmaf(us2f((unsigned short)dof[ks][e]),
                      us2f((unsigned short)of[ks][e]), dl);
    dl = at_sum4(dl);
    const int row = q0 + 16 * T.wid + T.g;
    const long srow = ((long)n * heads + h) * L + row;
    if (T.lg == 0 && row < L) delta[srow] = dl;
    const float lse2 = row < L ? lse[srow] * AT_LOG2E : 0.f;

    f32x4 acc[4] = {};
    auto tile = [&](int t, const bf16* ik, const bf16* iv)
                    __attribute__((always_inline)) {
        f32x4 ds[4];
        #pragma unroll
        for (int st = 0; st < 4; ++st) {
            f32x4 s = {}, dp = {};
            #pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                s = at_mma(at_frag(T, ik, st, ks), qf[ks], s);
                dp = at_mma(at_frag(T, iv, st, ks), dof[ks], dp);
            }
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = t * AT_T + 16 * st + 4 * T.lg + r;
                const float p = key < L
                    ? __builtin_amdgcn_exp2f(fmaf(s[r], AT_C2, -lse2)) : 0.f;
                ds[st][r] = p * (dp[r] - dl);
            }
        }
        #pragma unroll
        for (int c = 0; c < 2; ++c) {
            const at_bf16x8 df = at_pack8(ds[2 * c], ds[2 * c + 1]);
            #pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                acc[dt] = at_mma(at_frag_t(T, ik, c, dt), df, acc[dt]);
        }
    };
    auto issue = [&](int t, bf16* ik, bf16* iv) __attribute__((always_inline)) {
        at_stage(T, kb, ld, t * AT_T, L, ik);
        at_stage(T, vb, ld, t * AT_T, L, iv);
    };

    issue(0, img_k0, img_v0);
    for (int t = 0; t < nt; t += 2) {
        at_barrier();
        if (t + 1 < nt) issue(t + 1, img_k1, img_v1);
        tile(t, img_k0, img_v0);
        if (t + 1 >= nt) break;
        at_barrier();
        if (t + 2 < nt) issue(t + 2, img_k0, img_v0);
        tile(t + 1, img_k1, img_v1);
    }
    at_barrier();
    at_store_tile(T, acc, 0.125f, img_k0, dqkv + hoff, ld, q0, L);
}

// ------------------------------------------------------- backward dk, dv ---

// grid (ceil(L / 64), heads, N): the block's 64 keys, 16 per wave; streams
// the queries' q and do with their lse and delta
__global__ __launch_bounds__(AT_BLOCK)
void k_attn_bwd_dkv(const bf16* __restrict__ qkv, const bf16* __restrict__ dO,
                    const float* __restrict__ lse,
                    const float* __restrict__ delta, bf16* __restrict__ dqkv,
                    int L, int heads) {
    __shared__ __align__(16) bf16 img_q0[AT_IMG];
    __shared__ __align__(16) bf16 img_g0[AT_IMG];
    __shared__ __align__(16) bf16 img_q1[AT_IMG];
    __shared__ __align__(16) bf16 img_g1[AT_IMG];
    __shared__ __align__(16) float stat0[2 * AT_T];   // lse | delta
    __shared__ __align__(16) float stat1[2 * AT_T];
    const AtLane T = at_lane();
    const int D = heads * AT_D, ld = 3 * D;
    const int h = blockIdx.y, n = blockIdx.z, k0 = blockIdx.x * AT_T;
    const long hoff = (long)n * L * ld + h * AT_D;
    const bf16* qb = qkv + hoff;
    const bf16* gb = dO + (long)n * L * D + h * AT_D;
    // wave 0 brings a tile's lse, wave 1 its delta
    const float* stat_src =
        (T.wid == 0 ? lse : delta) + ((long)n * heads + h) * L;
    const int nt = (L + AT_T - 1) / AT_T;

    at_bf16x8 kf[2], vf[2];
    at_own(T, qkv + hoff + D, ld, k0, L, kf);
    at_own(T, qkv + hoff + 2 * D, ld, k0, L, vf);

    f32x4 dk[4] = {}, dv[4] = {};
    auto tile = [&](int t, const bf16* iq, const bf16* ig, const float* st_)
                    __attribute__((always_inline)) {
        f32x4 pp[4], ds[4];
        #pragma unroll
        for (int st = 0; st < 4; ++st) {
            f32x4 s = {}, dp = {};
            #pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                s = at_mma(at_frag(T, iq, st, ks), kf[ks], s);
                dp = at_mma(at_frag(T, ig, st, ks), vf[ks], dp);
            }
            const f32x4 ls = *reinterpret_cast<const f32x4*>(
                st_ + 16 * st + 4 * T.lg);
            const f32x4 dl = *reinterpret_cast<const f32x4*>(
                st_ + AT_T + 16 * st + 4 * T.lg);
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qr = t * AT_T + 16 * st + 4 * T.lg + r;
                const float p = qr < L
                    ? __builtin_amdgcn_exp2f(
                          fmaf(s[r], AT_C2, -(ls[r] * AT_LOG2E))) : 0.f;
                pp[st][r] = p;
                ds[st][r] = p * (dp[r] - dl[r]);
            }
        }
        #pragma unroll
        for (int c = 0; c < 2; ++c) {
            const at_bf16x8 pf = at_pack8(pp[2 * c], pp[2 * c + 1]);
            const at_bf16x8 df = at_pack8(ds[2 * c], ds[2 * c + 1]);
            #pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                dv[dt] = at_mma(at_frag_t(T, ig, c, dt), pf, dv[dt]);
                dk[dt] = at_mma(at_frag_t(T, iq, c, dt), df, dk[dt]);
            }
        }
    };
    // waves 0 and 1 also bring the tile's 64 lse and 64 delta, 4 B per lane
    auto issue = [&](int t, bf16* iq, bf16* ig, float* st_)
                     __attribute__((always_inline)) {
        at_stage(T, qb, ld, t * AT_T, L, iq);
        at_stage(T, gb, D, t * AT_T, L, ig);
        if (T.wid < 2) {
            const int qr = t * AT_T + T.lane;
            const unsigned long a = qr < L
                ? reinterpret_cast<unsigned long>(stat_src + qr)
                : T.zaddr;
            __builtin_amdgcn_global_load_lds(
                reinterpret_cast<at_glb_u32_ptr>(a),
                (at_lds_u32_ptr)(st_ + T.wid * AT_T), 4, 0, 0);
        }
    };

    issue(0, img_q0, img_g0, stat0);
    for (int t = 0; t < nt; t += 2) {
        at_barrier();
        if (t + 1 < nt) issue(t + 1, img_q1, img_g1, stat1);
        tile(t, img_q0, img_g0, stat0);
        if (t + 1 >= nt) break;
        at_barrier();
        if (t + 2 < nt) issue(t + 2, img_q0, img_g0, stat0);
        tile(t + 1, img_q1, img_g1, stat1);
    }
    at_barrier();
    at_store_tile(T, dk, 0.125f, img_q0, dqkv + hoff + D, ld, k0, L);
    at_store_tile(T, dv, 1.f, img_g0, dqkv + hoff + 2 * D, ld, k0, L);
}

// ------------------------------------------------------- position table ---

// y[n][i] = x[n][i] + pos[i] over 16 B chunks; per8 chunks per image
__global__ __launch_bounds__(AT_BLOCK)
void k_add_pos(const bf16* __restrict__ x, const bf16* __restrict__ pos,
               bf16* __restrict__ y, long n8, long per8) {
    const long step = (long)gridDim.x * AT_BLOCK;
    for (long i = (long)blockIdx.x * AT_BLOCK + threadIdx.x; i < n8;
         i += step) {
        const s16x8 a = *reinterpret_cast<const s16x8*>(x + i * 8);
        const s16x8 b = *reinterpret_cast<const s16x8*>(pos + (i % per8) * 8);
        s16x8 v;
        #pragma unroll
        for (int e = 0; e < 8; ++e)
            v[e] = at_f2bf_bits(us2f((unsigned short)a[e]) +
                                us2f((unsigned short)b[e]));
        *reinterpret_cast<s16x8*>(y + i * 8) = v;
    }
}

// ------------------------------------------------------------------ hosts ---

struct AtPlan { int tile, stream; dim3 grid; };

// The one host decision, a function of the shape alone.  All three kernels
// tile their own rows and the streamed rows by 64.
static AtPlan at_make_plan(long N, long heads, long L) {
    TORCH_CHECK(N >= 1 && heads >= 1 && L >= 1, "attn: empty problem");
    TORCH_CHECK(N <= 65535 && heads <= 65535,
                "attn: N and heads ride in grid.z / grid.y, at most 65535");
    // 32-bit element offsets inside one image row block, with a tile of slack
    TORCH_CHECK(N * (L + AT_T) * 3 * AT_D * heads < (1l << 31),
                "attn: qkv has 2^31 elements or more");
    AtPlan p;
    p.tile = AT_T;
    p.stream = AT_T;
    p.grid = dim3((unsigned)((L + AT_T - 1) / AT_T), (unsigned)heads,
                  (unsigned)N);
    return p;
}

std::tuple<long, long, long, long, long> attn_plan(const std::string& op,
                                                   long N, long heads, long L) {
    TORCH_CHECK(op == "fwd" || op == "bwd_dq" || op == "bwd_dkv",
                "attn_plan: op must be fwd, bwd_dq or bwd_dkv, got ", op);
    const AtPlan p = at_make_plan(N, heads, L);
    return {p.tile, p.stream, p.grid.x, p.grid.y, p.grid.z};
}

static void at_check_act(const at::Tensor& t, long C, const char* who,
                         const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
                t.dim() == 4, who, ": ", what, " must be bf16 [N,C,H,W]");
    TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast),
                who, ": ", what, " must be channels_last");
    TORCH_CHECK(t.size(1) == C, who, ": ", what, " needs ", C,
                " channels (64 per head), got ", t.size(1));
}

static at::Tensor at_empty(const at::Tensor& like, long C) {
    return at::empty({like.size(0), C, like.size(2), like.size(3)},
                     like.options().memory_format(
                         at::MemoryFormat::ChannelsLast));
}

static const bf16* at_cptr(const at::Tensor& t) {
    return reinterpret_cast<const bf16*>(t.data_ptr());
}
static bf16* at_ptr(at::Tensor& t) {
    return reinterpret_cast<bf16*>(t.data_ptr());
}

// (o, lse [N, heads, L]); lse is empty without `save`
std::tuple<at::Tensor, at::Tensor> attn_fwd(at::Tensor qkv, long heads,
                                            bool save) {
    TORCH_CHECK(heads >= 1, "attn_fwd: heads must be positive");
    const long D = AT_D * heads;
    at_check_act(qkv, 3 * D, "attn_fwd", "qkv");
    const long N = qkv.size(0), L = qkv.size(2) * qkv.size(3);
    const AtPlan p = at_make_plan(N, heads, L);
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto o = at_empty(qkv, D);
    auto lse = at::empty({save ? N : 0, heads, L},
                         qkv.options().dtype(at::kFloat));
    if (save)
        hipLaunchKernelGGL((k_attn_fwd<true>), p.grid, dim3(AT_BLOCK), 0,
                           stream, at_cptr(qkv), at_ptr(o),
                           lse.data_ptr<float>(), (int)L, (int)heads);
    else
        hipLaunchKernelGGL((k_attn_fwd<false>), p.grid, dim3(AT_BLOCK), 0,
                           stream, at_cptr(qkv), at_ptr(o), (float*)nullptr,
                           (int)L, (int)heads);
    HIP_CHECK_LAST();
    return {o, lse};
}

at::Tensor attn_bwd(at::Tensor qkv, at::Tensor o, at::Tensor lse,
                    at::Tensor dO, long heads) {
    TORCH_CHECK(heads >= 1, "attn_bwd: heads must be positive");
    const long D = AT_D * heads;
    at_check_act(qkv, 3 * D, "attn_bwd", "qkv");
    at_check_act(o, D, "attn_bwd", "o");
    at_check_act(dO, D, "attn_bwd", "do");
    const long N = qkv.size(0), L = qkv.size(2) * qkv.size(3);
    TORCH_CHECK(o.size(0) == N && o.size(2) == qkv.size(2) &&
                o.size(3) == qkv.size(3) && dO.sizes() == o.sizes(),
                "attn_bwd: o and do must be [N, D, H, W] of qkv's N, H, W");
    TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat &&
                lse.is_contiguous() && lse.numel() == N * heads * L,
                "attn_bwd: lse must be contiguous fp32 [N, heads, L] (a "
                "forward with save)");
    const AtPlan p = at_make_plan(N, heads, L);
    auto stream = at::hip::getCurrentHIPStream().stream();
    auto dqkv = at_empty(qkv, 3 * D);
    auto delta = at::empty_like(lse);
    hipLaunchKernelGGL(k_attn_bwd_dq, p.grid, dim3(AT_BLOCK), 0, stream,
                       at_cptr(qkv), at_cptr(o), at_cptr(dO),
                       lse.data_ptr<float>(), delta.data_ptr<float>(),
                       at_ptr(dqkv), (int)L, (int)heads);
    HIP_CHECK_LAST();
    hipLaunchKernelGGL(k_attn_bwd_dkv, p.grid, dim3(AT_BLOCK), 0, stream,
                       at_cptr(qkv), at_cptr(dO), lse.data_ptr<float>(),
                       delta.data_ptr<float>(), at_ptr(dqkv), (int)L,
                       (int)heads);
    HIP_CHECK_LAST();
    return dqkv;
}

// y = x + pos, pos [1, D, H, W] broadcast over N
at::Tensor add_pos_fwd(at::Tensor x, at::Tensor pos) {
    TORCH_CHECK(x.dim() == 4, "add_pos_fwd: x must be [N,C,H,W]");
    at_check_act(x, x.size(1), "add_pos_fwd", "x");
    at_check_act(pos, x.size(1), "add_pos_fwd", "pos");
    TORCH_CHECK(pos.size(0) == 1 && pos.size(2) == x.size(2) &&
                pos.size(3) == x.size(3),
                "add_pos_fwd: pos must be [1, C, H, W] of x's C, H, W");
    TORCH_CHECK(x.size(1) % 8 == 0 && x.numel() > 0,
                "add_pos_fwd: needs C % 8 == 0 and a non-empty x");
    const long n8 = x.numel() / 8, per8 = pos.numel() / 8;
    auto y = at_empty(x, x.size(1));
    hipLaunchKernelGGL(k_add_pos,
                       dim3(std::min<long>(AP_GRID,
                                           ceil_div_i(n8, AT_BLOCK))),
                       dim3(AT_BLOCK), 0,
                       at::hip::getCurrentHIPStream().stream(), at_cptr(x),
                       at_cptr(pos), at_ptr(y), n8, per8);
    HIP_CHECK_LAST();
    return y;
}
