// gemm.hip — bf16 MFMA GEMM family for the linear layers plus
// transpose / column-sum / slab-combine utilities shared with conv.
//
// Two kernels compute the same tiles, bit for bit:
//
// k_gemm_dma (the routed one, docs/KERNELS.md "Linear GEMM: LDS-DMA tiles"):
// operands staged by global_load_lds where they lie, either K-contiguous
// (x, w, dy as dgrad's A) or K-major (w as dgrad's B, dy and x for wgrad,
// fragments by ds_read_b64_tr_b16), two LDS image pairs so the next K-tile
// is in flight under the MFMAs, 16-B staged epilogue.  No transpose kernel
// runs on its paths.  plan_linear / linear_plan decide per product class;
// `impl` (-1 automatic, 0 legacy, 1 forced) and DDPX_LINEAR=0 override.
//
// k_gemm_tn (legacy; every shape the DMA kernel does not fit, i.e. a row
// length that is no multiple of 8, and impl 0): C[M,N] = A[M,K] · B[N,K]^T
// ("tn": both operands row-major, K fastest — the natural layout for X·W^T
// with torch Linear weights and, after a transpose_bf16 of the weight or of
// dy and x, for the dgrad/wgrad products).
//
// CDNA4 mapping: v_mfma_f32_16x16x32_bf16 per-wave tiles; 256-thread block
// = 4 waves in a 2×2 grid, each wave owns a 64×64 output sub-tile as 4×4
// fragments with fp32 accumulators in AGPRs.  LDS tiles are row-padded by
// 8 bf16 (16 B) so the 64-lane ds_read_b128 fragment reads are
// bank-conflict-free (row stride 144 B = 36 dwords; r*36 mod 64 covers
// distinct multiples of 4 — see cdna_hip_programming.md §6 Guideline 4).
// Split-K (grid.z) writes fp32 partial slabs, combined by a deterministic
// fixed-order reduction (no fp atomics anywhere).
//
// Epilogue modes (bf16 output only): EPI_RELU writes relu(acc + bias),
// EPI_RELU_DROP writes relu(acc + bias) * scale where the counter-hash mask
// (common.h) keeps the element and +0 where it drops it.  The mask is
// evaluated from the element's offset row*N + col and never stored; with
// split-K the epilogue runs in the combine kernel.  The per-call seed is
// the host's h(seed ^ DROP_SALT ^ rank*DROP_RANK_SALT, (epoch << 32) | calls)
// with DROP_SALT = 0xA0761D6478BD642F, DROP_RANK_SALT = 0xE7037ED1A0B428DB
// (mirror: ops/functional.py).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

typedef short bf16x8_t __attribute__((ext_vector_type(8)));

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int LDK = BK + 8;          // padded row length (bf16 elements)
constexpr int GEMM_THREADS = 256;

enum { EPI_NONE = 0, EPI_RELU = 1, EPI_RELU_DROP = 2 };

struct DropArgs {
    unsigned long long seed;   // per-call seed
    unsigned thr;              // drop when the 16 hashed bits are < thr
    float scale;               // 65536 / (65536 - thr)
};

// relu with NaN passed through and -0 -> +0
DEV_INLINE float relu_pos(float v) { return v <= 0.f ? 0.f : v; }

// The element epilogue of every full (non-slab) output, shared by k_gemm_tn
// and k_gemm_dma: bias, then ReLU, then the dropout mask of the element's
// offset row*N + col.  A slab entry passes through with badd = 0, EPI_NONE.
template <int EPI>
DEV_INLINE float gemm_epilogue(long row, int col, float acc, float badd,
                               int N, const DropArgs& drop) {
    float v = acc + badd;
    if (EPI != EPI_NONE) v = relu_pos(v);
    if (EPI == EPI_RELU_DROP) {
        v = drop_keep(drop.seed, row * N + col, drop.thr)
            ? __fmul_rn(v, drop.scale) : 0.f;
    }
    return v;
}

// ------------------------------------------------------------ core kernel ---

template <bool OUT_F32, bool SPLITK, int EPI = EPI_NONE>
__global__ __launch_bounds__(GEMM_THREADS)
void k_gemm_tn(const bf16* __restrict__ A, const bf16* __restrict__ B,
               const float* __restrict__ bias, void* __restrict__ Cout,
               int M, int N, int K, int k_per_split, DropArgs drop) {
    static_assert(EPI == EPI_NONE || (!OUT_F32 && !SPLITK),
                  "epilogue modes write the final bf16 tile");
    __shared__ bf16 lds_a[BM][LDK];
    __shared__ bf16 lds_b[BN][LDK];

    const int m0 = blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int kz0 = SPLITK ? blockIdx.z * k_per_split : 0;
    const int kz1 = SPLITK ? min(K, kz0 + k_per_split) : K;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;           // 4 waves: 2x2
    const int wr = wid >> 1;            // wave row (0..1) -> 64 rows each
    const int wc = wid & 1;             // wave col (0..1) -> 64 cols each

    f32x4 acc[4][4] = {};

    const int ld_row = tid >> 3;        // 32 rows per pass
    const int ld_col = (tid & 7) * 8;   // 8 segments of 8 bf16 = 16B

    for (int kt = kz0; kt < kz1; kt += BK) {
        // ---- stage A and B tiles (zero-fill out of range) ----
        #pragma unroll
        for (int p = 0; p < 4; ++p) {
            int row = p * 32 + ld_row;
            int gm = m0 + row, gk = kt + ld_col;
            bf16x8_t va = {};
            if (gm < M && gk + 7 < kz1) {
                va = *reinterpret_cast<const bf16x8_t*>(&A[(long)gm * K + gk]);
            } else if (gm < M) {
                for (int j = 0; j < 8; ++j) {
                    short v = 0;
                    if (gk + j < kz1) v = ((const short*)A)[(long)gm * K + gk + j];
                    va[j] = v;
                }
            }
            *reinterpret_cast<bf16x8_t*>(&lds_a[row][ld_col]) = va;

            int gn = n0 + row;
            bf16x8_t vb = {};
            if (gn < N && gk + 7 < kz1) {
                vb = *reinterpret_cast<const bf16x8_t*>(&B[(long)gn * K + gk]);
            } else if (gn < N) {
                for (int j = 0; j < 8; ++j) {
                    short v = 0;
                    if (gk + j < kz1) v = ((const short*)B)[(long)gn * K + gk + j];
                    vb[j] = v;
                }
            }
            *reinterpret_cast<bf16x8_t*>(&lds_b[row][ld_col]) = vb;
        }
        __syncthreads();

        // ---- MFMA over the staged BK in two 32-deep steps ----
        #pragma unroll
        for (int ks = 0; ks < BK; ks += 32) {
            bf16x8_t af[4], bf[4];
            const int kcol = ks + (lane >> 4) * 8;
            #pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                af[mi] = *reinterpret_cast<const bf16x8_t*>(
                    &lds_a[wr * 64 + mi * 16 + (lane & 15)][kcol]);
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                bf[ni] = *reinterpret_cast<const bf16x8_t*>(
                    &lds_b[wc * 64 + ni * 16 + (lane & 15)][kcol]);
            #pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                #pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
        }
        __syncthreads();
    }

    // ---- epilogue: D lane map col=lane&15, row=(lane>>4)*4+r ----
    #pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            int col = n0 + wc * 64 + ni * 16 + (lane & 15);
            if (col >= N) continue;
            float badd = (bias && !SPLITK) ? bias[col] : 0.f;
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                int row = m0 + wr * 64 + mi * 16 + (lane >> 4) * 4 + r;
                if (row >= M) continue;
                float v = gemm_epilogue<EPI>(row, col, acc[mi][ni][r], badd,
                                             N, drop);
                if (SPLITK) {
                    float* slab = reinterpret_cast<float*>(Cout);
                    slab[((long)blockIdx.z * M + row) * N + col] = v;
                } else if (OUT_F32) {
                    reinterpret_cast<float*>(Cout)[(long)row * N + col] = v;
                } else {
                    reinterpret_cast<bf16*>(Cout)[(long)row * N + col] =
                        f2bf(v);
                }
            }
        }
    }
}

// deterministic split-K combine: out[i] = bias-free fixed-order sum of slabs
// (+ bias).  The epilogue modes walk groups of four consecutive elements so
// one hash serves its whole group.
template <bool OUT_F32, int EPI = EPI_NONE>
__global__ void k_splitk_combine(const float* __restrict__ slab, int S,
                                 long MN, int N, const float* __restrict__ bias,
                                 void* __restrict__ out, DropArgs drop) {
    static_assert(EPI == EPI_NONE || !OUT_F32, "epilogue modes write bf16");
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long stride = (long)gridDim.x * blockDim.x;
    if (EPI == EPI_NONE) {
        for (; i < MN; i += stride) {
            float v = 0.f;
            for (int s = 0; s < S; ++s) v += slab[(long)s * MN + i];
            if (bias) v += bias[i % N];
            if (OUT_F32) reinterpret_cast<float*>(out)[i] = v;
            else reinterpret_cast<bf16*>(out)[i] = f2bf(v);
        }
        return;
    }
    const long groups = (MN + 3) >> 2;
    for (long g = i; g < groups; g += stride) {
        unsigned long long z = 0;
        if (EPI == EPI_RELU_DROP) z = drop_hash(drop.seed, (unsigned long long)g);
        const long e0 = g << 2;
        int col = (int)(e0 % N);
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long e = e0 + j;
            if (e >= MN) break;
            float v = 0.f;
            for (int s = 0; s < S; ++s) v += slab[(long)s * MN + e];
            if (bias) v += bias[col];
            if (++col == N) col = 0;
            v = relu_pos(v);
            if (EPI == EPI_RELU_DROP)
                v = drop_lane(z, (unsigned)j) >= drop.thr
                    ? __fmul_rn(v, drop.scale) : 0.f;
            reinterpret_cast<bf16*>(out)[e] = f2bf(v);
        }
    }
}

// ---------------------------------------------------------- LDS-DMA kernel ---

// Out-of-range staging lanes read these 16 zero bytes: global_load_lds has
// no mask that leaves LDS defined, and no lane forms an address outside its
// operand.
static __device__ __align__(16) unsigned char g_lin_zero16[16];

typedef short tr16x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) tr16x4_t* lds_tr16_ptr;
typedef __attribute__((address_space(3))) unsigned short* lds_u16_ptr;
typedef const __attribute__((address_space(1))) unsigned short* glb_u16_ptr;

// C[M,N] = sum_k A(m,k) * B(n,k), k_gemm_tn's tile, wave grid, split plan,
// K-tile order, k-to-lane mapping and MFMA order, so C is bit-identical to
// k_gemm_tn's on the same values.  What differs is how a tile reaches LDS
// and leaves it.
//
// Each operand is read where it lies, in one of two layouts:
//   contiguous (KMAJOR false): P[row * K + k], rows of the output dimension.
//     LDS image [128][64]; a 64-lane DMA chunk is 8 rows x 8 segments of 16 B,
//     physical segment = logical segment ^ (row & 7), applied to the source
//     address and again on the ds_read_b128 fragment read (conv_gemm_body's).
//   K-major (KMAJOR true): P[k * OUT + col], rows of k, output dimension
//     fastest (w for dgrad, dy and x for wgrad).  LDS image [64][128] in
//     memory order; a chunk is 4 k-rows x 16 segments, segment ^
//     2*((row & 3) | ((row >> 3) & 1) << 2); fragments come from
//     ds_read_b64_tr_b16, two reads 4 rows apart (k_conv_wgrad_wide_dma's
//     image, swizzle and read: lane group lane>>4 receives
//     k = ks + 8*(lane>>4) + j for output index lane&15).
// Staging is global_load_lds only, 16 B per lane.  Two image pairs: tile
// t+1 is in flight while tile t is multiplied, one barrier per tile (its
// vmcnt(0) lands tile t; every wave has left tile t-1's reads).  The four
// images are separate __shared__ objects so the compiler can tell a DMA into
// one pair from the fragment reads of the other.
//
// Epilogue: the dead images stage the tile (fp32: 32 rows per image, all
// four; bf16: 64 rows per image, two), 16 B chunks XOR-ed with the row's
// lane group so the fragment-order writes spread over the banks, then each
// thread writes 16 B of consecutive columns.
//
// Needs (plan_linear checks them): 16-B aligned operand rows and output
// rows, i.e. K % 8 == 0 for a contiguous operand, OUT % 8 == 0 for a K-major
// one, N % 8 == 0; k_per_split % 64 == 0 or == K (splitk_plan gives that).
// Block barrier that first lands this wave's in-flight global_load_lds.
// Spelled out: k_gemm_dma is NO_PK_F32, and a function without that
// attribute (__syncthreads) is not inlined into one that has it.
DEV_INLINE void dma_barrier() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <bool A_KMAJOR, bool B_KMAJOR, bool OUT_F32, bool SPLITK,
          int EPI = EPI_NONE>
__global__ __launch_bounds__(GEMM_THREADS, 2) NO_PK_F32
void k_gemm_dma(const bf16* __restrict__ A, const bf16* __restrict__ B,
                const float* __restrict__ bias, void* __restrict__ Cout,
                int M, int N, int K, int k_per_split, DropArgs drop) {
    static_assert(EPI == EPI_NONE || (!OUT_F32 && !SPLITK),
                  "epilogue modes write the final bf16 tile");
    __shared__ __align__(16) bf16 img_a0[BM * BK];
    __shared__ __align__(16) bf16 img_b0[BN * BK];
    __shared__ __align__(16) bf16 img_a1[BM * BK];
    __shared__ __align__(16) bf16 img_b1[BN * BK];

    const int m0 = blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int kz0 = SPLITK ? blockIdx.z * k_per_split : 0;
    const int kz1 = SPLITK && kz0 + k_per_split < K ? kz0 + k_per_split : K;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 1, wc = wid & 1;
    const int lg = lane >> 4;           // lane group: k octet / D row quad
    const int g = lane & 15;

    unsigned long zaddr = reinterpret_cast<unsigned long>(g_lin_zero16);
    asm volatile("" : "+s"(zaddr));

    // ---- staging state: wave wid fills chunks wid + 4i of each image; a
    // lane's source for chunk i is base + i * step (+ the tile's k offset).
    // kq: contiguous, the lane's k within a tile; K-major, its k row within
    // chunk 0.  ok[i]: the output-dimension bound of chunk i.
    auto src_init = [&](auto km, const bf16* P, int o0, int OUT,
                        unsigned long& base, long& step, int& kq,
                        bool (&ok)[4]) __attribute__((always_inline)) {
        if constexpr (decltype(km)::value) {
            const int lseg = g ^ (2 * (lg | (((wid >> 1) & 1) << 2)));
            const int oc = o0 + lseg * 8;
            kq = 4 * wid + lg;
            base = reinterpret_cast<unsigned long>(P)
                + (unsigned long)(((long)kq * OUT + oc) * (long)sizeof(bf16));
            step = (long)16 * OUT * (long)sizeof(bf16);
            #pragma unroll
            for (int i = 0; i < 4; ++i) ok[i] = oc < OUT;
        } else {
            const int pl_row = lane >> 3;
            const int row = wid * 8 + pl_row;
            kq = ((lane & 7) ^ pl_row) * 8;
            base = reinterpret_cast<unsigned long>(P)
                + (unsigned long)(((long)(o0 + row) * K + kq)
                                  * (long)sizeof(bf16));
            step = (long)32 * K * (long)sizeof(bf16);
            #pragma unroll
            for (int i = 0; i < 4; ++i) ok[i] = o0 + row + 32 * i < OUT;
        }
    };
    auto issue = [&](auto km, bf16* img, unsigned long base, long step,
                     int kq, const bool (&ok)[4], int kt, int OUT)
                     __attribute__((always_inline)) {
        constexpr bool KM = decltype(km)::value;
        const unsigned long tile = base + (unsigned long)(
            (KM ? (long)kt * OUT : (long)kt) * (long)sizeof(bf16));
        #pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool v = ok[i] && kt + kq + (KM ? 16 * i : 0) < kz1;
            const unsigned long addr =
                v ? tile + (unsigned long)(i * step) : zaddr;
            __builtin_amdgcn_global_load_lds(
                reinterpret_cast<glb_u16_ptr>(addr),
                (lds_u16_ptr)(img + (wid + 4 * i) * 512), 16, 0, 0);
        }
    };
    using AKM = std::integral_constant<bool, A_KMAJOR>;
    using BKM = std::integral_constant<bool, B_KMAJOR>;
    unsigned long a_base, b_base;
    long a_step, b_step;
    int a_kq, b_kq;
    bool a_ok[4], b_ok[4];
    src_init(AKM{}, A, m0, M, a_base, a_step, a_kq, a_ok);
    src_init(BKM{}, B, n0, N, b_base, b_step, b_kq, b_ok);
    auto issue_tile = [&](int kt, bf16* ia, bf16* ib)
                          __attribute__((always_inline)) {
        issue(AKM{}, ia, a_base, a_step, a_kq, a_ok, kt, M);
        issue(BKM{}, ib, b_base, b_step, b_kq, b_ok, kt, N);
    };

    // ---- fragment reads: element offsets, constant over tiles ----
    // K-major: lane addresses img[8*lg + (g>>2)][col0 + (g&3)*4], swizzled
    const int rsw = 2 * ((g >> 2) | ((lg & 1) << 2));
    const int rbase = (lg * 8 + (g >> 2)) * 128 + (g & 1) * 4;
    const int rseg = (g & 3) >> 1;
    int offa[4], offb[4];
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (A_KMAJOR) {
            offa[i] = rbase + ((wr * 8 + i * 2 + rseg) ^ rsw) * 8;
        } else {
            const int row = wr * 64 + i * 16 + g;
            offa[i] = row * BK + ((lg ^ (row & 7)) * 8);
        }
        if (B_KMAJOR) {
            offb[i] = rbase + ((wc * 8 + i * 2 + rseg) ^ rsw) * 8;
        } else {
            const int row = wc * 64 + i * 16 + g;
            offb[i] = row * BK + ((lg ^ (row & 7)) * 8);
        }
    }
    // contiguous: the 32-deep step ks moves the logical segment by 4, which
    // flips bit 2 of the physical one: offset ^ 32 elements
    auto frag = [&](auto km, const bf16* img, int off, int ks)
                    __attribute__((always_inline)) -> bf16x8_t {
        if constexpr (decltype(km)::value) {
            const bf16* p = img + ks * 128 + off;
            tr16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (lds_tr16_ptr)p);
            tr16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (lds_tr16_ptr)(p + 4 * 128));
            return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        } else {
            return *reinterpret_cast<const bf16x8_t*>(img + (off ^ ks));
        }
    };

    f32x4 acc[4][4] = {};
    auto mma_tile = [&](const bf16* ia, const bf16* ib)
                        __attribute__((always_inline)) {
        #pragma unroll
        for (int ks = 0; ks < BK; ks += 32) {
            bf16x8_t af[4], bfr[4];
            #pragma unroll
            for (int mi = 0; mi < 4; ++mi) af[mi] = frag(AKM{}, ia, offa[mi], ks);
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni) bfr[ni] = frag(BKM{}, ib, offb[ni], ks);
            #pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                #pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[mi], bfr[ni], acc[mi][ni], 0, 0, 0);
        }
    };

    // ---- K loop: ascending tiles, ping-pong images ----
    issue_tile(kz0, img_a0, img_b0);
    for (int kt = kz0; kt < kz1; kt += 2 * BK) {
        dma_barrier();     // tile kt landed; pair 1 is free
        if (kt + BK < kz1) issue_tile(kt + BK, img_a1, img_b1);
        mma_tile(img_a0, img_b0);
        if (kt + BK >= kz1) break;
        dma_barrier();
        if (kt + 2 * BK < kz1) issue_tile(kt + 2 * BK, img_a0, img_b0);
        mma_tile(img_a1, img_b1);
    }
    dma_barrier();       // every fragment read retired: images are stage

    // ---- epilogue: D lane map col = g, row = lg*4 + r ----
    float badd[4];
    #pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int col = n0 + wc * 64 + ni * 16 + g;
        badd[ni] = (!SPLITK && bias && col < N) ? bias[col] : 0.f;
    }
    if constexpr (OUT_F32 || SPLITK) {
        // fp32 stage [32][128] per image: rows 0-31 a0, 32-63 b0, 64-95 a1,
        // 96-127 b1; column ^ (lg << 4) with lg = (row >> 2) & 3
        #pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            bf16* img = (mi >> 1) ? (wr ? img_b1 : img_b0)
                                  : (wr ? img_a1 : img_a0);
            float* st = reinterpret_cast<float*>(img);
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int cl = wc * 64 + ni * 16 + g;
                const int col = n0 + cl;
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rloc = (mi & 1) * 16 + lg * 4 + r;
                    const long row = (long)m0 + wr * 64 + mi * 16 + lg * 4 + r;
                    st[rloc * 128 + (cl ^ (lg << 4))] =
                        gemm_epilogue<EPI_NONE>(row, col, acc[mi][ni][r],
                                                badd[ni], N, drop);
                }
            }
        }
        dma_barrier();
        float* outp = reinterpret_cast<float*>(Cout)
            + (SPLITK ? (long)blockIdx.z * M * N : 0L);
        const int csub = (tid & 31) * 4, rsub = tid >> 5;
        #pragma unroll
        for (int p = 0; p < 16; ++p) {
            const int rl = p * 8 + rsub;
            const long row = (long)m0 + rl;
            const int col = n0 + csub;
            const bf16* img = (p >> 3) ? ((p >> 2) & 1 ? img_b1 : img_a1)
                                       : ((p >> 2) & 1 ? img_b0 : img_a0);
            const float* st = reinterpret_cast<const float*>(img);
            if (row < M && col < N) {
                f32x4 v = *reinterpret_cast<const f32x4*>(
                    st + (rl & 31) * 128 + (csub ^ (((rl >> 2) & 3) << 4)));
                *reinterpret_cast<f32x4*>(outp + row * N + col) = v;
            }
        }
    } else {
        // bf16 stage [64][128] per image: rows 0-63 a0, 64-127 b0
        bf16* st = wr ? img_b0 : img_a0;
        #pragma unroll
        for (int mi = 0; mi < 4; ++mi)
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int cl = wc * 64 + ni * 16 + g;
                const int col = n0 + cl;
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rloc = mi * 16 + lg * 4 + r;
                    const long row = (long)m0 + wr * 64 + rloc;
                    st[rloc * 128 + (cl ^ (lg << 4))] =
                        f2bf(gemm_epilogue<EPI>(row, col, acc[mi][ni][r],
                                                badd[ni], N, drop));
                }
            }
        dma_barrier();
        bf16* outp = reinterpret_cast<bf16*>(Cout);
        const int csub = (tid & 15) * 8, rsub = tid >> 4;
        #pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int rl = p * 16 + rsub;
            const long row = (long)m0 + rl;
            const int col = n0 + csub;
            const bf16* src = (p >> 2) ? img_b0 : img_a0;
            if (row < M && col < N) {
                s16x8 v = *reinterpret_cast<const s16x8*>(
                    src + (rl & 63) * 128 + (csub ^ (((rl >> 2) & 3) << 4)));
                *reinterpret_cast<s16x8*>(outp + row * N + col) = v;
            }
        }
    }
}

// ----------------------------------------------- small-N / small-K kernels ---

// C[M,N] = A[M,K] · B[N,K]^T for tiny N (<=16): thread per (m,n), vec8 K loop
__global__ void k_gemm_tn_smalln(const bf16* __restrict__ A,
                                 const bf16* __restrict__ B,
                                 const float* __restrict__ bias,
                                 bf16* __restrict__ C, int M, int N, int K) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)M * N) return;
    int n = i % N;
    long m = i / N;
    const bf16* a = A + m * K;
    const bf16* b = B + (long)n * K;
    float acc = 0.f;
    int k = 0;
    for (; k + 8 <= K; k += 8) {
        bf16x8_t va = *reinterpret_cast<const bf16x8_t*>(&a[k]);
        bf16x8_t vb = *reinterpret_cast<const bf16x8_t*>(&b[k]);
        #pragma unroll
        for (int j = 0; j < 8; ++j)
            acc = fmaf(us2f((unsigned short)va[j]), us2f((unsigned short)vb[j]), acc);
    }
    for (; k < K; ++k) acc = fmaf(bf2f(a[k]), bf2f(b[k]), acc);
    if (bias) acc += bias[n];
    C[i] = f2bf(acc);
}

// C[M,N] = A[M,K] · B[K,N] for tiny K: thread per (m, 8-wide n chunk)
__global__ void k_gemm_nn_smallk(const bf16* __restrict__ A,
                                 const bf16* __restrict__ B,
                                 bf16* __restrict__ C, int M, int N, int K) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long nv = N / 8;
    if (i >= (long)M * nv) return;
    int nb = (i % nv) * 8;
    long m = i / nv;
    float acc[8] = {};
    for (int k = 0; k < K; ++k) {
        float a = bf2f(A[m * K + k]);
        bf16x8_t vb = *reinterpret_cast<const bf16x8_t*>(&B[(long)k * N + nb]);
        #pragma unroll
        for (int j = 0; j < 8; ++j)
            acc[j] = fmaf(a, us2f((unsigned short)vb[j]), acc[j]);
    }
    bf16x8_t o;
    #pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (short)f2us(acc[j]);
    *reinterpret_cast<bf16x8_t*>(&C[m * N + nb]) = o;
}

// dW[N,K] += dY^T·X for tiny N: grid.z splits over M into fp32 slab
__global__ void k_wgrad_smalln(const bf16* __restrict__ dY,
                               const bf16* __restrict__ X,
                               float* __restrict__ slab,
                               int M, int N, int K, int S) {
    int s = blockIdx.z;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long kv = K / 8;
    if (i >= (long)N * kv) return;
    int kb = (i % kv) * 8;
    int n = i / kv;
    float acc[8] = {};
    for (long m = s; m < M; m += S) {
        float g = bf2f(dY[m * N + n]);
        bf16x8_t vx = *reinterpret_cast<const bf16x8_t*>(&X[m * K + kb]);
        #pragma unroll
        for (int j = 0; j < 8; ++j)
            acc[j] = fmaf(g, us2f((unsigned short)vx[j]), acc[j]);
    }
    float* out = slab + ((long)s * N + n) * K + kb;
    #pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = acc[j];
}

// ------------------------------------------------------------- transposes ---

// bf16 2D transpose: out[j,i] = in[i,j]; 32x32 LDS tiles (+1 pad)
__global__ void k_transpose_bf16(const bf16* __restrict__ in,
                                 bf16* __restrict__ out, int R, int Ccols) {
    __shared__ bf16 tile[32][33];
    int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    int tc = threadIdx.x % 32, tr = threadIdx.x / 32;  // 256 thr: 32x8
    #pragma unroll
    for (int rr = 0; rr < 32; rr += 8) {
        int r = r0 + tr + rr, c = c0 + tc;
        tile[tr + rr][tc] = (r < R && c < Ccols) ? in[(long)r * Ccols + c]
                                                 : f2bf(0.f);
    }
    __syncthreads();
    #pragma unroll
    for (int rr = 0; rr < 32; rr += 8) {
        int r = r0 + tc, c = c0 + tr + rr;   // write transposed
        if (r < R && c < Ccols)
            out[(long)c * R + r] = tile[tc][tr + rr];
    }
}

// -------------------------------------------------------------- column sum ---

// colsum[c] = sum_m in[m][c] (bf16 in, fp32 out), deterministic slab
// scheme, bf16x8-vectorized; slab layout [C][S] so combine waves read each
// channel's splits coalesced.
// C = column-window width (<= 2048); ldx = full row stride, so wide
// matrices (e.g. the VGG classifier's 4096-wide bias grad) sweep in
// column windows
__global__ void k_colsum_partial(const bf16* __restrict__ x, long M, int C,
                                 long ldx, int S, float* __restrict__ slab) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* red = reinterpret_cast<float*>(smem);   // [nw][C]
    const int cpg = C >> 3;
    const int c8 = threadIdx.x % cpg;
    const int walker = threadIdx.x / cpg;
    const int nw = blockDim.x / cpg;
    const int s = blockIdx.x;
    float acc[8] = {};
    for (long r = (long)s * nw + walker; r < M; r += (long)S * nw) {
        s16x8 v = reinterpret_cast<const s16x8*>(x + r * ldx)[c8];
        #pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += us2f((unsigned short)v[j]);
    }
    #pragma unroll
    for (int j = 0; j < 8; ++j) red[walker * C + c8 * 8 + j] = acc[j];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float t = 0.f;
        for (int w = 0; w < nw; ++w) t += red[w * C + c];
        slab[(long)c * S + s] = t;
    }
}

// scalar fallback for C % 8 != 0 (tiny tensors, e.g. the 10-class head)
__global__ void k_colsum_partial_scalar(const bf16* __restrict__ x, long M,
                                        int C, int S, float* __restrict__ slab) {
    int c = threadIdx.x % C;
    int walker = threadIdx.x / C;
    int nw = blockDim.x / C;
    int s = blockIdx.x;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* red = reinterpret_cast<float*>(smem);   // [nw][C]
    float sum = 0.f;
    if (walker < nw) {
        for (long r = (long)s * nw + walker; r < M; r += (long)S * nw)
            sum += bf2f(x[r * C + c]);
        red[walker * C + c] = sum;
    }
    __syncthreads();
    for (int cc = threadIdx.x; cc < C; cc += blockDim.x) {
        float t = 0.f;
        for (int w = 0; w < nw; ++w) t += red[w * C + cc];
        slab[(long)cc * S + s] = t;
    }
}

__global__ void k_colsum_combine(const float* __restrict__ slab, int S, int C,
                                 float* __restrict__ out) {
    int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (c >= C) return;
    float v = 0.f;
    for (int s = lane; s < S; s += 64) v += slab[(long)c * S + s];
    v = wave_reduce_sum(v);
    if (lane == 0) out[c] = v;
}

// --------------------------------------------------- relu+dropout backward ---

// dz = bf16(float(dy) * scale) where y > 0, else +0.  y is the fused
// forward's output: scale >= 1, so y > 0 exactly where the element was kept
// and its pre-activation was positive; no mask is read or regenerated.
// aligned: both pointers 16-byte aligned (s16x8 body), else all scalar.
__global__ void k_relu_drop_bwd(const bf16* __restrict__ dy,
                                const bf16* __restrict__ y,
                                bf16* __restrict__ dz, long n, float scale,
                                int aligned) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long stride = (long)gridDim.x * blockDim.x;
    long nv = aligned ? (n >> 3) : 0;
    for (long v = i; v < nv; v += stride) {
        s16x8 g = reinterpret_cast<const s16x8*>(dy)[v];
        s16x8 a = reinterpret_cast<const s16x8*>(y)[v];
        s16x8 o;
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
            float d = __fmul_rn(us2f((unsigned short)g[j]), scale);
            o[j] = us2f((unsigned short)a[j]) > 0.f ? (short)f2us(d) : (short)0;
        }
        reinterpret_cast<s16x8*>(dz)[v] = o;
    }
    for (long j = nv * 8 + i; j < n; j += stride) {
        float d = __fmul_rn(bf2f(dy[j]), scale);
        dz[j] = bf2f(y[j]) > 0.f ? f2bf(d) : f2bf(0.f);
    }
}

// ------------------------------------------------------------------ hosts ---

// split-K when the tile grid underfills the 256-CU chip; returns the number
// of splits and the BK-aligned K range of each
static int splitk_plan(int gm, int gn, int K, int& k_per_split) {
    int S = 1;
    while (gm * gn * S < 512 && S < 16 && (K / (S * 2)) >= BK) S *= 2;
    k_per_split = K;
    if (S > 1) {
        k_per_split = ceil_div_i(K, S);
        k_per_split = ((k_per_split + BK - 1) / BK) * BK;
        S = ceil_div_i(K, k_per_split);  // recompute actual
    }
    return S;
}

// ---- one host decision: LDS-DMA kernel or the legacy path ----

// LIN_GEMM: a plain gemm_tn call, the forward class without the small-N
// kernels in front of it
enum { LIN_FWD = 0, LIN_DGRAD = 1, LIN_WGRAD = 2, LIN_GEMM = 3 };

// DDPX_LINEAR=0 (read once per process) keeps the automatic plan on legacy
static bool linear_env_off() {
    static const bool off = [] {
        const char* e = std::getenv("DDPX_LINEAR");
        return e != nullptr && e[0] == '0' && e[1] == '\0';
    }();
    return off;
}

// automatic routing per product class, decided by tools/bench_kernels.py
// --linear (docs/KERNELS.md "Linear GEMM: LDS-DMA tiles")
static const bool LIN_ROUTE_DMA[3] = {true, true, true};

// k_gemm_dma's shape needs for C[M,N] contracting K, whichever layout its
// operands have: every operand row and output row is N or K elements long
// (the contraction length of a contiguous operand, the output dimension of
// a K-major one), so both must be multiples of 8 (16 B)
static bool dma_fits(long N, long K) {
    return N > 0 && K > 0 && N % 8 == 0 && K % 8 == 0;
}

// the DMA reads 16 B per lane: a view whose storage offset breaks that
// alignment stays on the legacy kernel
static bool aligned16(const at::Tensor& a, const at::Tensor& b) {
    return (((uintptr_t)a.data_ptr() | (uintptr_t)b.data_ptr()) & 15) == 0;
}

static void check_impl(long impl) {
    TORCH_CHECK(impl >= -1 && impl <= 1, "impl must be -1 (automatic), 0 "
                "(legacy) or 1 (LDS-DMA), got ", impl);
}

// Pure arithmetic.  (M, N, K) are the linear layer's: batch, out features,
// in features.  Every class stages rows of length N (dy, or the y it
// writes) and rows of length K (x, w, dx, dw), so all need N % 8 == 0 and
// K % 8 == 0; N <= 16 belongs to the small kernels.
static bool plan_linear(int op, long M, long N, long K, long impl) {
    check_impl(impl);
    TORCH_CHECK(op >= LIN_FWD && op <= LIN_GEMM, "op must be 0 (fwd), 1 "
                "(dgrad), 2 (wgrad) or 3 (gemm_tn), got ", op);
    if (impl == 0 || M <= 0 || !dma_fits(N, K)) return false;
    if (op != LIN_GEMM && N <= 16) return false;
    if (impl == 1) return true;
    return LIN_ROUTE_DMA[op == LIN_GEMM ? LIN_FWD : op] && !linear_env_off();
}

std::string linear_plan(long op, long M, long N, long K, long impl) {
    return plan_linear((int)op, M, N, K, impl) ? "dma" : "legacy";
}

template <bool AKM, bool BKM, bool OUT_F32, bool SPLITK, int EPI = EPI_NONE>
static void launch_dma(hipStream_t stream, dim3 grid, const bf16* a,
                       const bf16* b, const float* bp, void* c, int M, int N,
                       int K, int kps, DropArgs drop) {
    hipLaunchKernelGGL((k_gemm_dma<AKM, BKM, OUT_F32, SPLITK, EPI>), grid,
                       dim3(GEMM_THREADS), 0, stream, a, b, bp, c, M, N, K,
                       kps, drop);
}
template <bool OUT_F32, bool SPLITK, int EPI = EPI_NONE>
static void launch_tn(hipStream_t stream, dim3 grid, const bf16* a,
                      const bf16* b, const float* bp, void* c, int M, int N,
                      int K, int kps, DropArgs drop) {
    hipLaunchKernelGGL((k_gemm_tn<OUT_F32, SPLITK, EPI>), grid,
                       dim3(GEMM_THREADS), 0, stream, a, b, bp, c, M, N, K,
                       kps, drop);
}

// Operand layouts of a k_gemm_dma launch.  Only the instantiations a linear
// layer needs exist: forward (both contiguous, every output mode), dgrad
// (A contiguous, B K-major, bf16 out), wgrad (both K-major, fp32 out).
enum { LAY_TN = 0, LAY_DGRAD = 1, LAY_WGRAD = 2 };

// C[M,N] = A x B contracting K, split-K by splitk_plan, slabs combined by
// k_splitk_combine.  dma: k_gemm_dma on the operands as `lay` describes
// them; else k_gemm_tn on A [M,K], B [N,K].
// epi: EPI_NONE for every plain product; the ReLU / ReLU+dropout modes are
// linear_act_fwd's and need a bf16 C
static void launch_gemm(const at::Tensor& A, const at::Tensor& B,
                        const c10::optional<at::Tensor>& bias, at::Tensor& C,
                        int M, int N, int K, bool out_f32, bool dma,
                        int lay = LAY_TN, int epi = EPI_NONE,
                        DropArgs drop = DropArgs{0ull, 0u, 1.0f}) {
    auto stream = at::hip::getCurrentHIPStream().stream();
    const bf16* a = reinterpret_cast<const bf16*>(A.data_ptr());
    const bf16* b = reinterpret_cast<const bf16*>(B.data_ptr());
    const float* bp = bias.has_value() ? bias->data_ptr<float>() : nullptr;
    TORCH_CHECK(epi == EPI_NONE || !out_f32);
    TORCH_CHECK(dma || lay == LAY_TN);
    TORCH_CHECK(lay == LAY_TN || (epi == EPI_NONE && !bp &&
                                  out_f32 == (lay == LAY_WGRAD)));
    if (dma)
        TORCH_CHECK((((uintptr_t)a | (uintptr_t)b | (uintptr_t)C.data_ptr())
                     & 15) == 0, "LDS-DMA GEMM: operands 16-byte aligned");

    int gm = ceil_div_i(M, BM), gn = ceil_div_i(N, BN);
    int k_per_split;
    int S = splitk_plan(gm, gn, K, k_per_split);
    if (S > 1) {
        auto slab = at::empty({S, M, N}, A.options().dtype(at::kFloat));
        float* sp = slab.data_ptr<float>();
        dim3 grid(gm, gn, S);
        if (!dma)
            launch_tn<false, true>(stream, grid, a, b, nullptr, sp, M, N, K,
                                   k_per_split, drop);
        else if (lay == LAY_TN)
            launch_dma<false, false, false, true>(stream, grid, a, b, nullptr,
                                                  sp, M, N, K, k_per_split,
                                                  drop);
        else if (lay == LAY_DGRAD)
            launch_dma<false, true, false, true>(stream, grid, a, b, nullptr,
                                                 sp, M, N, K, k_per_split,
                                                 drop);
        else
            launch_dma<true, true, false, true>(stream, grid, a, b, nullptr,
                                                sp, M, N, K, k_per_split,
                                                drop);
        HIP_CHECK_LAST();
        long MN = (long)M * N;
        int blocks = std::min<long>(4096, ceil_div_i(MN, 256));
        if (out_f32)
            hipLaunchKernelGGL(k_splitk_combine<true>, dim3(blocks), dim3(256),
                               0, stream, sp, S, MN, N, bp, C.data_ptr(),
                               drop);
        else if (epi == EPI_NONE)
            hipLaunchKernelGGL(k_splitk_combine<false>, dim3(blocks), dim3(256),
                               0, stream, sp, S, MN, N, bp, C.data_ptr(),
                               drop);
        else {
            // four elements per thread
            blocks = std::min<long>(4096, ceil_div_i((MN + 3) / 4, 256));
            if (epi == EPI_RELU)
                hipLaunchKernelGGL((k_splitk_combine<false, EPI_RELU>),
                                   dim3(blocks), dim3(256), 0, stream, sp, S,
                                   MN, N, bp, C.data_ptr(), drop);
            else
                hipLaunchKernelGGL((k_splitk_combine<false, EPI_RELU_DROP>),
                                   dim3(blocks), dim3(256), 0, stream, sp, S,
                                   MN, N, bp, C.data_ptr(), drop);
        }
        HIP_CHECK_LAST();
        return;
    }
    dim3 grid(gm, gn, 1);
    void* c = C.data_ptr();
    if (!dma) {
        if (out_f32)
            launch_tn<true, false>(stream, grid, a, b, bp, c, M, N, K, K, drop);
        else if (epi == EPI_NONE)
            launch_tn<false, false>(stream, grid, a, b, bp, c, M, N, K, K,
                                    drop);
        else if (epi == EPI_RELU)
            launch_tn<false, false, EPI_RELU>(stream, grid, a, b, bp, c, M, N,
                                              K, K, drop);
        else
            launch_tn<false, false, EPI_RELU_DROP>(stream, grid, a, b, bp, c,
                                                   M, N, K, K, drop);
    } else if (lay == LAY_DGRAD) {
        launch_dma<false, true, false, false>(stream, grid, a, b, bp, c, M, N,
                                              K, K, drop);
    } else if (lay == LAY_WGRAD) {
        launch_dma<true, true, true, false>(stream, grid, a, b, bp, c, M, N,
                                            K, K, drop);
    } else if (out_f32) {
        launch_dma<false, false, true, false>(stream, grid, a, b, bp, c, M, N,
                                              K, K, drop);
    } else if (epi == EPI_NONE) {
        launch_dma<false, false, false, false>(stream, grid, a, b, bp, c, M,
                                               N, K, K, drop);
    } else if (epi == EPI_RELU) {
        launch_dma<false, false, false, false, EPI_RELU>(
            stream, grid, a, b, bp, c, M, N, K, K, drop);
    } else {
        launch_dma<false, false, false, false, EPI_RELU_DROP>(
            stream, grid, a, b, bp, c, M, N, K, K, drop);
    }
    HIP_CHECK_LAST();
}

at::Tensor gemm_tn(at::Tensor A, at::Tensor B, c10::optional<at::Tensor> bias,
                   bool out_f32, long impl) {
    TORCH_CHECK(A.is_cuda() && A.scalar_type() == at::kBFloat16 &&
                A.is_contiguous());
    TORCH_CHECK(B.is_cuda() && B.scalar_type() == at::kBFloat16 &&
                B.is_contiguous());
    TORCH_CHECK(A.size(1) == B.size(1), "K mismatch");
    int M = A.size(0), N = B.size(0), K = A.size(1);
    auto C = at::empty({M, N}, A.options().dtype(out_f32 ? at::kFloat
                                                         : at::kBFloat16));
    const bool dma = plan_linear(LIN_GEMM, M, N, K, impl) && aligned16(A, B);
    launch_gemm(A, B, bias, C, M, N, K, out_f32, dma);
    return C;
}

at::Tensor transpose_bf16(at::Tensor x) {
    TORCH_CHECK(x.dim() == 2 && x.scalar_type() == at::kBFloat16 &&
                x.is_contiguous());
    int R = x.size(0), C = x.size(1);
    auto out = at::empty({C, R}, x.options());
    auto stream = at::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(k_transpose_bf16,
                       dim3(ceil_div_i(C, 32), ceil_div_i(R, 32)), dim3(256),
                       0, stream.stream(),
                       reinterpret_cast<const bf16*>(x.data_ptr()),
                       reinterpret_cast<bf16*>(out.data_ptr()), R, C);
    HIP_CHECK_LAST();
    return out;
}

at::Tensor col_sum(at::Tensor x) {
    // x viewed as [M, C] bf16 (rows contiguous); returns fp32 [C]
    TORCH_CHECK(x.dim() == 2 && x.scalar_type() == at::kBFloat16 &&
                x.is_contiguous());
    long M = x.size(0);
    int C = x.size(1);
    auto stream = at::hip::getCurrentHIPStream();
    auto out = at::empty({C}, x.options().dtype(at::kFloat));
    if (C % 8 == 0) {
        // column windows of <= 2048 (one window for every model head up
        // to that width; the VGG 4096-wide classifier takes two)
        for (int c0 = 0; c0 < C; c0 += 2048) {
            int Cw = std::min(2048, C - c0);
            int cpg = Cw / 8;
            int block = (256 / cpg) * cpg;
            if (block == 0) block = cpg;     // cpg in (128, 256]: 1 walker
            int nw = std::max(1, block / cpg);
            int S = (int)std::max<long>(1, std::min<long>(1024, M / (nw * 4)));
            auto slab = at::empty({Cw, S}, x.options().dtype(at::kFloat));
            hipLaunchKernelGGL(k_colsum_partial, dim3(S), dim3(block),
                               nw * Cw * 4, stream.stream(),
                               reinterpret_cast<const bf16*>(x.data_ptr()) + c0,
                               M, Cw, (long)C, S, slab.data_ptr<float>());
            HIP_CHECK_LAST();
            hipLaunchKernelGGL(k_colsum_combine, dim3(ceil_div_i(Cw, 4)),
                               dim3(256), 0, stream.stream(),
                               slab.data_ptr<float>(), S, Cw,
                               out.data_ptr<float>() + c0);
            HIP_CHECK_LAST();
        }
        return out;
    }
    TORCH_CHECK(C <= 256, "col_sum scalar path needs C<=256");
    int nw = 256 / C;
    int block = nw * C;
    int S = (int)std::max<long>(1, std::min<long>(512, M / (nw * 4)));
    auto slab = at::empty({C, S}, x.options().dtype(at::kFloat));
    hipLaunchKernelGGL(k_colsum_partial_scalar, dim3(S), dim3(block),
                       nw * C * 4, stream.stream(),
                       reinterpret_cast<const bf16*>(x.data_ptr()), M, C, S,
                       slab.data_ptr<float>());
    HIP_CHECK_LAST();
    hipLaunchKernelGGL(k_colsum_combine, dim3(ceil_div_i(C, 4)), dim3(256), 0,
                       stream.stream(), slab.data_ptr<float>(), S, C,
                       out.data_ptr<float>());
    HIP_CHECK_LAST();
    return out;
}

// --------------------------------------------------------- linear wrappers ---

static void check_linear_operand(const at::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.dim() == 2 &&
                t.scalar_type() == at::kBFloat16 && t.is_contiguous(),
                name, ": contiguous cuda bf16 matrix");
}

at::Tensor linear_fwd(at::Tensor x, at::Tensor w,
                      c10::optional<at::Tensor> bias, long impl) {
    // x [M,K] bf16, w [N,K] bf16, bias fp32 -> y [M,N] bf16
    int M = x.size(0), N = w.size(0), K = x.size(1);
    check_impl(impl);
    auto stream = at::hip::getCurrentHIPStream();
    if (N <= 16) {
        auto y = at::empty({M, N}, x.options());
        long total = (long)M * N;
        int blocks = ceil_div_i(total, 256);
        const float* bp = bias.has_value() ? bias->data_ptr<float>() : nullptr;
        hipLaunchKernelGGL(k_gemm_tn_smalln, dim3(blocks), dim3(256), 0,
                           stream.stream(),
                           reinterpret_cast<const bf16*>(x.data_ptr()),
                           reinterpret_cast<const bf16*>(w.data_ptr()), bp,
                           reinterpret_cast<bf16*>(y.data_ptr()), M, N, K);
        HIP_CHECK_LAST();
        return y;
    }
    return gemm_tn(x, w, bias, /*out_f32=*/false, impl);
}

// elementwise.hip
at::Tensor relu_dropout_fwd(at::Tensor x, long thr, double scale,
                            long call_seed);

static void check_drop_args(long thr, double scale) {
    TORCH_CHECK(thr >= 0 && thr <= 65535, "dropout threshold ", thr,
                " outside [0, 65535]");
    TORCH_CHECK(thr != 0 || scale == 1.0, "thr == 0 needs scale == 1");
}

at::Tensor linear_act_fwd(at::Tensor x, at::Tensor w,
                          c10::optional<at::Tensor> bias, long thr,
                          double scale, long call_seed, long impl) {
    // y [M,N] bf16 = dropout(relu(x·w^T + bias)); thr == 0 is ReLU alone.
    // call_seed carries the 64 seed bits (as int64).
    check_drop_args(thr, scale);
    TORCH_CHECK(x.is_cuda() && x.dim() == 2 &&
                x.scalar_type() == at::kBFloat16 && x.is_contiguous());
    TORCH_CHECK(w.is_cuda() && w.dim() == 2 &&
                w.scalar_type() == at::kBFloat16 && w.is_contiguous());
    TORCH_CHECK(x.size(1) == w.size(1), "K mismatch");
    TORCH_CHECK(!bias.has_value() ||
                (bias->is_cuda() && bias->scalar_type() == at::kFloat &&
                 bias->is_contiguous() && bias->numel() == w.size(0)),
                "bias: contiguous cuda fp32 [N]");
    int M = x.size(0), N = w.size(0), K = x.size(1);
    check_impl(impl);
    if (N <= 16)    // small-N kernel, then the elementwise epilogue
        return relu_dropout_fwd(linear_fwd(x, w, bias, impl), thr, scale,
                                call_seed);
    auto y = at::empty({M, N}, x.options());
    DropArgs drop{(unsigned long long)call_seed, (unsigned)thr, (float)scale};
    launch_gemm(x, w, bias, y, M, N, K, /*out_f32=*/false,
                plan_linear(LIN_FWD, M, N, K, impl) && aligned16(x, w), LAY_TN,
                thr == 0 ? EPI_RELU : EPI_RELU_DROP, drop);
    return y;
}

at::Tensor relu_drop_bwd(at::Tensor dy, at::Tensor y, double scale) {
    TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16 &&
                dy.is_contiguous() && y.is_cuda() &&
                y.scalar_type() == at::kBFloat16 && y.is_contiguous() &&
                dy.sizes() == y.sizes(),
                "relu_drop_bwd: contiguous cuda bf16 dy and y of one shape");
    auto dz = at::empty_like(dy);
    long n = dy.numel();
    if (n == 0) return dz;
    int aligned = (((uintptr_t)dy.data_ptr() | (uintptr_t)y.data_ptr() |
                    (uintptr_t)dz.data_ptr()) & 15) == 0;
    int blocks = (int)std::min<long>(4096, ceil_div_i(ceil_div_i(n, 8), 256));
    auto stream = at::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(k_relu_drop_bwd, dim3(blocks), dim3(256), 0,
                       stream.stream(),
                       reinterpret_cast<const bf16*>(dy.data_ptr()),
                       reinterpret_cast<const bf16*>(y.data_ptr()),
                       reinterpret_cast<bf16*>(dz.data_ptr()), n,
                       (float)scale, aligned);
    HIP_CHECK_LAST();
    return dz;
}

at::Tensor linear_dgrad(at::Tensor dy, at::Tensor w, long impl) {
    // dy [M,N] bf16, w [N,K] -> dx [M,K] = dy·w
    int M = dy.size(0), N = dy.size(1), K = w.size(1);
    check_impl(impl);
    auto stream = at::hip::getCurrentHIPStream();
    if (N <= 16) {           // tiny contraction: nn-smallk over w directly
        TORCH_CHECK(K % 8 == 0);
        auto dx = at::empty({M, K}, dy.options());
        long total = (long)M * (K / 8);
        int blocks = ceil_div_i(total, 256);
        hipLaunchKernelGGL(k_gemm_nn_smallk, dim3(blocks), dim3(256), 0,
                           stream.stream(),
                           reinterpret_cast<const bf16*>(dy.data_ptr()),
                           reinterpret_cast<const bf16*>(w.data_ptr()),
                           reinterpret_cast<bf16*>(dx.data_ptr()), M, K, N);
        HIP_CHECK_LAST();
        return dx;
    }
    if (plan_linear(LIN_DGRAD, M, N, K, impl) && aligned16(dy, w)) {
        // A = dy rows (contraction n fastest), B = w as it lies: rows of
        // the contraction n, output k fastest
        check_linear_operand(dy, "dy");
        check_linear_operand(w, "w");
        TORCH_CHECK(w.size(0) == N, "dy / w shape mismatch");
        auto dx = at::empty({M, K}, dy.options());
        launch_gemm(dy, w, c10::nullopt, dx, M, K, N, /*out_f32=*/false,
                    /*dma=*/true, LAY_DGRAD);
        return dx;
    }
    auto wt = transpose_bf16(w);                  // [K,N]
    return gemm_tn(dy, wt, c10::nullopt, false, 0);  // [M,K]
}

at::Tensor linear_wgrad(at::Tensor dy, at::Tensor x, long impl) {
    // dy [M,N], x [M,K] -> dw fp32 [N,K] = dy^T·x
    int M = dy.size(0), N = dy.size(1), K = x.size(1);
    check_impl(impl);
    auto stream = at::hip::getCurrentHIPStream();
    if (N <= 16) {
        TORCH_CHECK(K % 8 == 0);
        int S = 32;
        auto slab = at::empty({S, N, K}, dy.options().dtype(at::kFloat));
        long total = (long)N * (K / 8);
        int blocks = ceil_div_i(total, 256);
        hipLaunchKernelGGL(k_wgrad_smalln, dim3(blocks, 1, S), dim3(256), 0,
                           stream.stream(),
                           reinterpret_cast<const bf16*>(dy.data_ptr()),
                           reinterpret_cast<const bf16*>(x.data_ptr()),
                           slab.data_ptr<float>(), M, N, K, S);
        HIP_CHECK_LAST();
        auto dw = at::empty({N, K}, dy.options().dtype(at::kFloat));
        long MN = (long)N * K;
        int cblocks = std::min<long>(4096, ceil_div_i(MN, 256));
        hipLaunchKernelGGL(k_splitk_combine<true>, dim3(cblocks), dim3(256), 0,
                           stream.stream(), slab.data_ptr<float>(), S, MN, K,
                           nullptr, dw.data_ptr(), DropArgs{0ull, 0u, 1.0f});
        HIP_CHECK_LAST();
        return dw;
    }
    if (plan_linear(LIN_WGRAD, M, N, K, impl) && aligned16(dy, x)) {
        // both operands as they lie: rows of the contraction m
        check_linear_operand(dy, "dy");
        check_linear_operand(x, "x");
        TORCH_CHECK(x.size(0) == M, "dy / x shape mismatch");
        auto dw = at::empty({N, K}, dy.options().dtype(at::kFloat));
        launch_gemm(dy, x, c10::nullopt, dw, N, K, M, /*out_f32=*/true,
                    /*dma=*/true, LAY_WGRAD);
        return dw;
    }
    auto dyt = transpose_bf16(dy);  // [N,M]
    auto xt = transpose_bf16(x);    // [K,M]
    return gemm_tn(dyt, xt, c10::nullopt, /*out_f32=*/true, 0);  // [N,K] fp32
}
