// conv.hip — NHWC implicit-GEMM convolutions on MFMA.
//
// Layout: activations bf16 channels_last (NHWC), weights bf16 KRSC.
// Forward treats conv as C[M=N·P·Q, Ko] = im2col(x)[M, R·S·C] · W[Ko, RSC]^T
// with the im2col gather done on the fly into LDS — channels are the
// fastest dim so the gathers are 16-byte vectors whenever C % 8 == 0.
// Backward-data is the same structure over dy with transformed weights
// WT2[C, R·S·Ko] (built once per step from the bf16 weight cache);
// backward-weight contracts over M with LDS-transposed staging and a
// fixed-order split-K slab reduction (deterministic, no atomics).
// conv1-style Cin<8 layers take a direct VALU path (MFMA starved at K=9 —
// SURVEY §2.4 note).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <climits>
#include <string>
#include <tuple>
#include <type_traits>
#include "common.h"

typedef short bf16x8_t __attribute__((ext_vector_type(8)));

constexpr int CBM = 128, CBK = 64;

struct ConvShape {
    int N, H, W, C;     // input
    int Ko, R, S;       // weights
    int P, Q;           // output
    int stride, pad;
    // magic-division decoders for the gathers (set on host)
    FastDiv fdQ, fdP, fdW, fdH, fdC, fdS, fdKo;
    // MODE 2 (strided dgrad, sub-grid class (a,b)): only taps whose
    // stride-residue matches the class contribute, so Kgemm shrinks to
    // nr*ns*Ko and no MFMA work is spent on zero taps.
    int cls_a, cls_b, nr, ns;
    int taps_r[4], taps_s[4];   // contributing (r, s) values
    int off_r[4], off_s[4];     // p = h' + off_r[ri], q = w' + off_s[si]
    int Hfull, Wfull;           // original dx dims (epilogue scatter)
    FastDiv fdNs;
    // MODE 1 tap-uniform row order (TAPS): GEMM rows run (group, pixel,
    // image-in-group) with G = 1 << lgG images per group; fdGHW divides by
    // G*H*W.
    FastDiv fdGHW;
    int lgG;
};

static inline void init_fastdiv(ConvShape& cs) {
    cs.fdQ.init(cs.Q); cs.fdP.init(cs.P); cs.fdW.init(cs.W);
    cs.fdH.init(cs.H); cs.fdC.init(cs.C); cs.fdS.init(cs.S);
    cs.fdKo.init(cs.Ko);
    cs.fdGHW.init(1); cs.lgG = 0;
}

// Tap-uniform dgrad rows (TAPS): the (r, s) taps that land inside dy for at
// least one dx pixel among GEMM rows [m_first, m_last]; bit r*S + s.  Rows
// decode as grp = m / GHW, pix = (m % GHW) >> lgG, so a tile inside one image
// group covers the contiguous pixel range [pix0, pix1]; a tile that crosses
// a group boundary takes the whole image.  Tap (r, s) reaches dy from pixel
// (h, w) iff 0 <= h + pad - r < P and 0 <= w + pad - s < Q.  ONE function for
// the kernel's K-loop mask and the host's tile count (conv2d_dgrad_plan).
__host__ __device__ inline unsigned dgrad_tap_mask(
        int m_first, int m_last, int GHW, int lgG, int H, int W, int P, int Q,
        int R, int S, int pad) {
    const int g0 = m_first / GHW, g1 = m_last / GHW;
    int pix0 = 0, pix1 = H * W - 1;
    if (g0 == g1) {
        pix0 = (m_first - g0 * GHW) >> lgG;
        pix1 = (m_last - g0 * GHW) >> lgG;
    }
    const int h0 = pix0 / W, h1 = pix1 / W;
    unsigned mask = 0;
    for (int h = h0; h <= h1; ++h) {
        // columns of this image row inside the pixel range
        const int wa = h == h0 ? pix0 - h0 * W : 0;
        const int wb = h == h1 ? pix1 - h1 * W : W - 1;
        const int ra = h + pad - P + 1 > 0 ? h + pad - P + 1 : 0;
        const int rb = h + pad < R - 1 ? h + pad : R - 1;
        const int sa = wa + pad - Q + 1 > 0 ? wa + pad - Q + 1 : 0;
        const int sb = wb + pad < S - 1 ? wb + pad : S - 1;
        for (int r = ra; r <= rb; ++r)
            for (int sx = sa; sx <= sb; ++sx)
                mask |= 1u << (r * S + sx);
    }
    return mask;
}

// ---------------------------------------------------------------- forward ---

// Unified implicit-GEMM kernel.  MODE 0 = forward (A gathered from x with
// k = (r,s,c)); MODE 1 = backward-data (A gathered from dy with
// k = (r,s,ko), B = WT2).  TBN selects the output-channel tile width
// (128, or 64 for narrow outputs like dgrad into C=64); the 256-thread
// block is WAVES_M x WAVES_N waves each owning a (128/WAVES_M) x
// (TBN/WAVES_N) sub-tile.
//
// Staging is __builtin_amdgcn_global_load_lds (direct HBM->LDS, 16 B/lane,
// no VGPR round trip — cdna_hip_programming.md §5 step 3: +69% on the GEMM
// ladder).  glds writes lane-linear, so the bank-conflict swizzle lives on
// the per-lane SOURCE address and is repeated on the fragment reads
// (rule 21): physical 16B segment = logical k-segment ^ (row & 7), which
// caps ds_read_b128 conflicts at 2-way on the 128 B rows.  Out-of-range
// lanes are pointed at a zeroed device buffer (glds has no execution mask
// that leaves LDS deterministic).
__device__ __align__(16) unsigned char g_zero16[16];

// Producer-side BN-backward fusion (MODE 1): the dgrad output dx IS the
// upstream BN's dy; while the staged epilogue streams dx out, it also
// accumulates that BN's backward partial sums (sum(dy_eff) and
// sum(dy_eff * xhat)) so the BN's own partial pass — a full re-read of
// x and dy — is skipped.
struct BnFuse {
    const bf16* x;                  // BN input (bf16 channels_last)
    const unsigned char* mask;      // packed relu mask (byte per 8 ch)
    const float* mean;
    const float* invstd;
    float* slab;                    // [2][C][gridM]
};

// The GEMM body lives in a __device__ function so two launchers can share
// it: k_conv_gemm (one ConvShape per launch) and k_conv_gemm_cls (MODE-2
// strided dgrad with blockIdx.z = residue class, one launch for ALL
// classes — VERDICT r01 next-round #7).  ``addin`` is an optional second
// operand streamed into the output epilogue (dx += addin): the ResNet
// skip-gradient accumulation fused into the junction conv's dgrad
// (VERDICT r01 next-round #4).
//
// WALK (MODE 0, and stride-1 MODE 1): the contraction channels (C forward,
// Ko dgrad) are a multiple of CBK, so every K-tile lies inside one tap and
// (r, s, channel base) are block-uniform.  The K loop then carries them as
// scalars; a lane's source is a per-lane 64-bit byte offset cached once
// (tap (0,0), its own channel segment) plus the tile's scalar tap offset,
// and the bounds test is two adds and two unsigned compares.  No division,
// no 64-bit multiply and no branch per chunk; LDS images, K-tile order and
// MFMA order are those of the decode loop, so outputs are bit-identical.
template <int MODE, int TBN, int WAVES_M, int WAVES_N, bool STRIDE1,
          int CBM_T, bool TAPS = false, bool WALK = false>
__device__ __forceinline__
void conv_gemm_body(const bf16* __restrict__ Asrc,
                    const bf16* __restrict__ Bsrc,
                    const float* __restrict__ bias, bf16* __restrict__ out,
                    const ConvShape& cs, int M, int Kgemm, int Nout,
                    float* __restrict__ stats, BnFuse bn,
                    const bf16* __restrict__ addin) {
    constexpr int WM = CBM_T / WAVES_M;
    constexpr int WN = TBN / WAVES_N;
    constexpr int MI = WM / 16;
    constexpr int NI = WN / 16;
    constexpr int A_CHUNKS = CBM_T / 8;    // 1 KiB glds chunks (8 rows)
    constexpr int B_CHUNKS = TBN / 8;
    // Single-buffer glds staging.  A 2-buffer prefetch ring was tried and
    // REVERTED: doubling LDS (64 KB) halved resident blocks/CU and measured
    // 10-30% SLOWER at every conv shape — this kernel hides HBM latency
    // with block-level parallelism (grids >> 256 workgroups), unlike the
    // guide's 256^2-tile GEMM that runs ~1 block/CU.
    __shared__ bf16 lds_a[1][CBM_T][CBK];  // unpadded: glds dest is linear
    __shared__ bf16 lds_b[1][TBN][CBK];
    static_assert(!TAPS || (MODE == 1 && STRIDE1), "TAPS is stride-1 dgrad");
    static_assert(!WALK || MODE == 0 || (MODE == 1 && STRIDE1),
                  "WALK is forward or stride-1 dgrad");
    // TAPS: consecutive blockIdx.x land on different XCDs (b and b + 8 share
    // one), so where the tile count divides, hand XCD j the j-th eighth of
    // the tiles — the blocks resident on one XCD then walk neighbouring
    // pixels of one image group and share their dy reads in that XCD's L2.
    // Measured: without it conv4 at G = 128 is 264.8 us, with it 230.5.
    const int tile_m = TAPS && (gridDim.x & 7) == 0
        ? (int)(blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3)
        : (int)blockIdx.x;
    const int m0 = tile_m * CBM_T;
    const int n0 = blockIdx.y * TBN;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int wr = wid / WAVES_N, wc = wid % WAVES_N;

    f32x4 acc[MI][NI] = {};
    // per-lane piece within a wave chunk: 8 rows x 8 segments of 16 B
    const int pl_row = lane >> 3;
    const int pl_segp = lane & 7;          // physical segment (LDS-linear)

    // Each thread's A-gather rows are FIXED across every k-tile (the chunk
    // assignment depends only on wid/lane), so the m-side decode runs ONCE
    // into registers; loops are fully unrolled so the per-row array keeps
    // CONSTANT indices (a runtime-indexed version spilled to scratch and
    // ran 40-100% slower — kept here as the measured counterexample).
    constexpr int A_PER = A_CHUNKS / 4;
    long ri_nb[A_PER];
    int ri_u[A_PER], ri_v[A_PER];
    // WALK: byte offset of the chunk's source at tap (0,0), channel segment
    // seg = pl_segp ^ pl_row (the same in every chunk: chunk rows are
    // multiples of 8 apart), and the row-valid predicate.  The wave index is
    // made provably uniform so chunk indices and LDS targets are scalars.
    long a_off[A_PER];
    bool a_rv[A_PER];
    const int walk_seg8 = (pl_segp ^ pl_row) * 8;
    const int widu = WALK ? __builtin_amdgcn_readfirstlane(wid) : wid;
    #pragma unroll
    for (int ci = 0; ci < A_PER; ++ci) {
        const int ch = wid + ci * 4;
        const int row = ch * 8 + pl_row;
        const int gm = m0 + row;
        ri_u[ci] = INT_MIN;
        if (WALK) { ri_v[ci] = 0; a_off[ci] = 0; a_rv[ci] = false; }
        if (gm < M) {
            if (MODE == 0) {
                unsigned rem = fd_div(gm, cs.fdQ);
                int q = fd_mod(gm, cs.fdQ, rem);
                unsigned n = fd_div(rem, cs.fdP);
                int p = fd_mod(rem, cs.fdP, n);
                ri_nb[ci] = (long)n * cs.H;
                ri_u[ci] = p * cs.stride - cs.pad;   // h0
                ri_v[ci] = q * cs.stride - cs.pad;   // w0
            } else if (MODE == 2) {
                unsigned rem = fd_div(gm, cs.fdW);
                int w1 = fd_mod(gm, cs.fdW, rem);
                unsigned n = fd_div(rem, cs.fdH);
                int h1 = fd_mod(rem, cs.fdH, n);
                ri_nb[ci] = (long)n * cs.P;
                ri_u[ci] = h1;
                ri_v[ci] = w1;
            } else if (TAPS) {
                // (group, pixel, image-in-group) order: see dgrad_tap_mask
                unsigned grp = fd_div(gm, cs.fdGHW);
                unsigned rem = fd_mod(gm, cs.fdGHW, grp);
                unsigned pix = rem >> cs.lgG;
                unsigned n = (grp << cs.lgG) + (rem & ((1u << cs.lgG) - 1));
                unsigned h = fd_div(pix, cs.fdW);
                int wcol = fd_mod(pix, cs.fdW, h);
                ri_nb[ci] = (long)n * cs.P;
                ri_u[ci] = (int)h + cs.pad;
                ri_v[ci] = wcol + cs.pad;
            } else {
                unsigned rem = fd_div(gm, cs.fdW);
                int wcol = fd_mod(gm, cs.fdW, rem);
                unsigned n = fd_div(rem, cs.fdH);
                int h = fd_mod(rem, cs.fdH, n);
                ri_nb[ci] = (long)n * cs.P;
                ri_u[ci] = h + cs.pad;
                ri_v[ci] = wcol + cs.pad;
            }
            if (WALK) {
                a_rv[ci] = true;
                a_off[ci] = (((ri_nb[ci] + ri_u[ci]) * (MODE == 0 ? cs.W : cs.Q)
                              + ri_v[ci]) * (MODE == 0 ? cs.C : cs.Ko)
                             + walk_seg8) * (long)sizeof(bf16);
            }
        }
    }
    // WALK B side: a lane's row of chunk 0 and its segment are fixed; chunk
    // bi is 32 rows (a block-uniform stride) further.
    constexpr int B_PER = B_CHUNKS / 4;
    long b_off = 0;
    bool b_cv[B_PER];
    if (WALK) {
        b_off = ((long)(n0 + widu * 8 + pl_row) * Kgemm + walk_seg8)
                * (long)sizeof(bf16);
        #pragma unroll
        for (int bi = 0; bi < B_PER; ++bi)
            b_cv[bi] = n0 + (widu + bi * 4) * 8 + pl_row < Nout;
    }
    // the zero buffer's address, held in SGPRs (opaque to the compiler, or
    // it re-materialises the address at every use)
    unsigned long zaddr = reinterpret_cast<unsigned long>(g_zero16);
    if (WALK) asm volatile("" : "+s"(zaddr));

    // One K-tile of the WALK loop: tap (r, sx), channel base c0, all scalar.
    auto issue_tile_walk = [&](int kt, int r, int sx, int c0, auto nopad_c) {
        constexpr bool NOPAD = decltype(nopad_c)::value;
        const int tap_off = MODE == 0 ? (r * cs.W + sx) * cs.C + c0
                                      : c0 - (r * cs.Q + sx) * cs.Ko;
        const unsigned long abase = reinterpret_cast<unsigned long>(Asrc)
            + (unsigned long)((long)tap_off * (long)sizeof(bf16));
        #pragma unroll
        for (int ci = 0; ci < A_PER; ++ci) {
            bool ok;
            if (NOPAD)          // MODE 0, pad == 0: every tap of a row is inside
                ok = a_rv[ci];
            else if (MODE == 0)
                ok = (unsigned)ri_u[ci] + (unsigned)r < (unsigned)cs.H &&
                     (unsigned)ri_v[ci] + (unsigned)sx < (unsigned)cs.W;
            else
                ok = (unsigned)ri_u[ci] - (unsigned)r < (unsigned)cs.P &&
                     (unsigned)ri_v[ci] - (unsigned)sx < (unsigned)cs.Q;
            const unsigned long addr =
                ok ? abase + (unsigned long)a_off[ci] : zaddr;
            __builtin_amdgcn_global_load_lds(
                reinterpret_cast<const __attribute__((address_space(1)))
                                 unsigned short*>(addr),
                (__attribute__((address_space(3))) unsigned short*)
                    &lds_a[0][(widu + ci * 4) * 8][0],
                16, 0, 0);
        }
        const unsigned long bbase = reinterpret_cast<unsigned long>(Bsrc)
            + (unsigned long)((long)kt * (long)sizeof(bf16));
        #pragma unroll
        for (int bi = 0; bi < B_PER; ++bi) {
            const unsigned long addr = b_cv[bi]
                ? bbase + (unsigned long)((long)bi * 32 * Kgemm
                                          * (long)sizeof(bf16))
                      + (unsigned long)b_off
                : zaddr;
            __builtin_amdgcn_global_load_lds(
                reinterpret_cast<const __attribute__((address_space(1)))
                                 unsigned short*>(addr),
                (__attribute__((address_space(3))) unsigned short*)
                    &lds_b[0][(widu + bi * 4) * 8][0],
                16, 0, 0);
        }
    };

    auto issue_tile = [&](int kt, int buf) {
        // ---- A tile: chunks round-robined over the 4 waves ----
        #pragma unroll
        for (int ci = 0; ci < A_PER; ++ci) {
            const int ch = wid + ci * 4;
            int row = ch * 8 + pl_row;
            int seg = pl_segp ^ (row & 7);     // logical k-segment
            int gk = kt + seg * 8;
            const bf16* src = reinterpret_cast<const bf16*>(g_zero16);
            if (ri_u[ci] != INT_MIN && gk < Kgemm) {
                if (MODE == 0) {
                    unsigned rs = fd_div(gk, cs.fdC);
                    int c = fd_mod(gk, cs.fdC, rs);
                    int r = fd_div(rs, cs.fdS);
                    int sx = fd_mod(rs, cs.fdS, r);
                    int h = ri_u[ci] + r;
                    int wcol = ri_v[ci] + sx;
                    if (h >= 0 && h < cs.H && wcol >= 0 && wcol < cs.W)
                        src = &Asrc[((ri_nb[ci] + h) * cs.W + wcol) * cs.C + c];
                } else if (MODE == 2) {
                    unsigned rs2 = fd_div(gk, cs.fdKo);
                    int ko = fd_mod(gk, cs.fdKo, rs2);
                    int ti = fd_div(rs2, cs.fdNs);
                    int si = fd_mod(rs2, cs.fdNs, ti);
                    int p = ri_u[ci] + cs.off_r[ti];
                    int q = ri_v[ci] + cs.off_s[si];
                    if (p >= 0 && p < cs.P && q >= 0 && q < cs.Q)
                        src = &Asrc[((ri_nb[ci] + p) * cs.Q + q) * cs.Ko + ko];
                } else if (STRIDE1) {
                    unsigned rs = fd_div(gk, cs.fdKo);
                    int ko = fd_mod(gk, cs.fdKo, rs);
                    int r = fd_div(rs, cs.fdS);
                    int sx = fd_mod(rs, cs.fdS, r);
                    int p = ri_u[ci] - r;
                    int q = ri_v[ci] - sx;
                    if (p >= 0 && p < cs.P && q >= 0 && q < cs.Q)
                        src = &Asrc[((ri_nb[ci] + p) * cs.Q + q) * cs.Ko + ko];
                } else {
                    unsigned rs = fd_div(gk, cs.fdKo);
                    int ko = fd_mod(gk, cs.fdKo, rs);
                    int r = fd_div(rs, cs.fdS);
                    int sx = fd_mod(rs, cs.fdS, r);
                    int pn = ri_u[ci] - r;
                    int qn = ri_v[ci] - sx;
                    int p = pn / cs.stride, q = qn / cs.stride;
                    if (pn >= 0 && qn >= 0 && pn == p * cs.stride &&
                        qn == q * cs.stride && p < cs.P && q < cs.Q)
                        src = &Asrc[((ri_nb[ci] + p) * cs.Q + q) * cs.Ko + ko];
                }
            }
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) unsigned short*)src,
                (__attribute__((address_space(3))) unsigned short*)&lds_a[buf][ch * 8][0],
                16, 0, 0);
        }
        // ---- B tile (row-contiguous source) ----
        for (int ch = wid; ch < B_CHUNKS; ch += 4) {
            int row = ch * 8 + pl_row;
            int seg = pl_segp ^ (row & 7);
            int gn = n0 + row, gk = kt + seg * 8;
            const bf16* src = reinterpret_cast<const bf16*>(g_zero16);
            if (MODE == 2) {
                // full wt2 row is R*S*Ko wide; map the class k-index to it
                if (gn < Nout && gk < Kgemm) {
                    unsigned rs2 = fd_div(gk, cs.fdKo);
                    int ko = fd_mod(gk, cs.fdKo, rs2);
                    int ri = fd_div(rs2, cs.fdNs);
                    int si = fd_mod(rs2, cs.fdNs, ri);
                    long gk_full = ((long)cs.taps_r[ri] * cs.S
                                    + cs.taps_s[si]) * cs.Ko + ko;
                    src = &Bsrc[(long)gn * (cs.R * cs.S * cs.Ko) + gk_full];
                }
            } else if (gn < Nout && gk < Kgemm)
                src = &Bsrc[(long)gn * Kgemm + gk];
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) unsigned short*)src,
                (__attribute__((address_space(3))) unsigned short*)&lds_b[buf][ch * 8][0],
                16, 0, 0);
        }
    };

    constexpr int buf = 0;
    // TAPS: Ko % 64 == 0, so every K-tile lies inside one tap.  The mask is
    // block-uniform (SGPRs): a tap no pixel of this tile reaches is stepped
    // over whole, both barriers with it.  The K-tiles that remain run in the
    // raster kernel's order, and a skipped one only added 0 * w.
    unsigned tap_mask = 0;
    if (TAPS)
        tap_mask = __builtin_amdgcn_readfirstlane(dgrad_tap_mask(
            m0, min(m0 + CBM_T, M) - 1, (int)cs.fdGHW.d, cs.lgG, cs.H, cs.W,
            cs.P, cs.Q, cs.R, cs.S, cs.pad));
    // the MFMA phase of one K-tile, shared by both loops
    auto mma_tile = [&]() {
        __syncthreads();   // vmcnt(0) for the in-flight glds + barrier
        #pragma unroll
        for (int ks = 0; ks < CBK; ks += 32) {
            bf16x8_t af[MI], bfr[NI];
            const int kgrp = (ks >> 3) + (lane >> 4);
            #pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                int row = wr * WM + mi * 16 + (lane & 15);
                af[mi] = *reinterpret_cast<const bf16x8_t*>(
                    &lds_a[buf][row][(kgrp ^ (row & 7)) * 8]);
            }
            #pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                int row = wc * WN + ni * 16 + (lane & 15);
                bfr[ni] = *reinterpret_cast<const bf16x8_t*>(
                    &lds_b[buf][row][(kgrp ^ (row & 7)) * 8]);
            }
            #pragma unroll
            for (int mi = 0; mi < MI; ++mi)
                #pragma unroll
                for (int ni = 0; ni < NI; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[mi], bfr[ni], acc[mi][ni], 0, 0, 0);
        }
        __syncthreads();
    };
    // WALK: one tap state (r, sx, c0, tap = r*S + sx), all scalar, serves
    // the tile's addresses and the TAPS skip.  K-tiles run in the decode
    // loop's order: c0 fastest, then sx, then r.
    auto walk_loop = [&](auto nopad_c) {
        const int Cd = MODE == 0 ? cs.C : cs.Ko;
        int kt = 0, tap = 0;
        for (int r = 0; r < cs.R; ++r)
            for (int sx = 0; sx < cs.S; ++sx, ++tap, kt += Cd) {
                if (TAPS && !((tap_mask >> tap) & 1u)) continue;
                for (int c0 = 0; c0 < Cd; c0 += CBK) {
                    issue_tile_walk(kt + c0, r, sx, c0, nopad_c);
                    mma_tile();
                }
            }
    };
    if (WALK) {
        // pad == 0 forward: block-uniform choice of the loop without the
        // bounds test
        if (MODE == 0 && cs.pad == 0) walk_loop(std::true_type{});
        else walk_loop(std::false_type{});
    } else {
        int tap = 0, tap_end = cs.Ko;   // [tap_end - Ko, tap_end) is tap's k
        for (int kt = 0; kt < Kgemm; kt += CBK) {
            if (TAPS) {
                if (kt == tap_end) { ++tap; tap_end += cs.Ko; }
                if (!((tap_mask >> tap) & 1u)) { kt = tap_end - CBK; continue; }
            }
            issue_tile(kt, 0);
            mma_tile();
        }
    }

    float psum[NI] = {}, psq[NI] = {};
    #pragma unroll
    for (int mi = 0; mi < MI; ++mi)
        #pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            int col = n0 + wc * WN + ni * 16 + (lane & 15);
            if (col >= Nout) continue;
            float badd = bias ? bias[col] : 0.f;
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                int row = m0 + wr * WM + mi * 16 + (lane >> 4) * 4 + r;
                if (row >= M) continue;
                if (MODE == 0 && stats) {
                    float v = acc[mi][ni][r] + badd;
                    psum[ni] += v;
                    psq[ni] = fmaf(v, v, psq[ni]);
                }
                if (MODE == 2) {
                    // scatter the class sub-grid back into full dx:
                    // (n, h', w') -> (a + h'*stride, b + w'*stride)
                    unsigned rem = fd_div(row, cs.fdW);
                    int w1 = fd_mod(row, cs.fdW, rem);
                    unsigned n = fd_div(rem, cs.fdH);
                    int h1 = fd_mod(rem, cs.fdH, n);
                    long addr = (((long)n * cs.Hfull + cs.cls_a
                                  + (long)h1 * cs.stride) * cs.Wfull
                                 + cs.cls_b + (long)w1 * cs.stride) * Nout
                                + col;
                    out[addr] = f2bf(acc[mi][ni][r] + badd);
                }
            }
        }

    if (MODE != 2) {
        // Coalesced epilogue: the fragment layout's direct stores are
        // scalar bf16 scattered across rows (32 B effective segments);
        // round-trip the tile through LDS and write full 16 B chunks of
        // consecutive columns instead.
        __syncthreads();                    // tiles are dead; reuse as stage
        // [CBM_T][TBN] image split across the two tile arrays (each holds
        // CBM_T*CBK elements; the image may need both)
        bf16* stageA = &lds_a[0][0][0];
        bf16* stageB = &lds_b[0][0][0];
        constexpr int HALF = CBM_T * CBK;
        auto stage_at = [&](int i) -> bf16& {
            return i < HALF ? stageA[i] : stageB[i - HALF];
        };
        #pragma unroll
        for (int mi = 0; mi < MI; ++mi)
            #pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                int cl = wc * WN + ni * 16 + (lane & 15);
                float badd2 = (bias && n0 + cl < Nout) ? bias[n0 + cl] : 0.f;
                #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    int rl = wr * WM + mi * 16 + (lane >> 4) * 4 + r;
                    stage_at(rl * TBN + cl) = f2bf(acc[mi][ni][r] + badd2);
                }
            }
        __syncthreads();
        // write phase: each 16-lane group streams one row's TBN columns.
        // With bn.slab set (MODE 1), the same sweep accumulates the
        // upstream BN's backward partials from the in-flight dx chunks.
        constexpr int ROWS_PER_PASS = 256 / (TBN / 8);
        const int rsub = tid / (TBN / 8);
        const int csub = (tid % (TBN / 8)) * 8;
        const bool do_bn = MODE == 1 && bn.slab != nullptr;
        float bsum[8] = {}, bsx[8] = {};
        float bmean[8], binv[8];
        if (do_bn && n0 + csub < Nout) {
            #pragma unroll
            for (int j = 0; j < 8; ++j) {
                bmean[j] = bn.mean[n0 + csub + j];
                binv[j] = bn.invstd[n0 + csub + j];
            }
        }
        for (int r0_ = 0; r0_ < CBM_T; r0_ += ROWS_PER_PASS) {
            int rl = r0_ + rsub;
            long row = (long)m0 + rl;
            int col = n0 + csub;
            const bool live = rl < CBM_T && row < M && col < Nout;
            if (TAPS && live) {
                // GEMM row -> physical dx row (n*H*W + pix)
                unsigned gm = (unsigned)row;
                unsigned grp = fd_div(gm, cs.fdGHW);
                unsigned rem = fd_mod(gm, cs.fdGHW, grp);
                unsigned n = (grp << cs.lgG) + (rem & ((1u << cs.lgG) - 1));
                row = (long)n * (cs.H * cs.W) + (rem >> cs.lgG);
            }
            if (live) {
                int i = rl * TBN + csub;    // 16 B chunk within one half
                const bf16* src16 = i < HALF ? &stageA[i] : &stageB[i - HALF];
                bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(src16);
                if (MODE == 1 && addin) {
                    // fused skip-grad accumulation: dx += addin (the
                    // junction's dresid), one inline read instead of a
                    // separate ATen add pass over dx+addin+out
                    s16x8 a8 = *reinterpret_cast<const s16x8*>(
                        &addin[row * Nout + col]);
                    s16x8& vv = reinterpret_cast<s16x8&>(v);
                    #pragma unroll
                    for (int j = 0; j < 8; ++j)
                        vv[j] = (short)f2us(us2f((unsigned short)vv[j])
                                            + us2f((unsigned short)a8[j]));
                }
                *reinterpret_cast<bf16x8_t*>(&out[row * Nout + col]) = v;
                if (do_bn) {
                    // mask byte of GLOBAL channel group col/8 (col = n0 +
                    // csub: blockIdx.y > 0 tiles must not reuse group 0's)
                    unsigned m8 = bn.mask
                        ? bn.mask[row * (Nout >> 3) + (col >> 3)] : 0xffu;
                    s16x8 xv = *reinterpret_cast<const s16x8*>(
                        &bn.x[row * Nout + col]);
                    #pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float g = (m8 >> j) & 1u
                            ? us2f((unsigned short)((s16x8&)v)[j]) : 0.f;
                        float xh = (us2f((unsigned short)xv[j]) - bmean[j])
                                   * binv[j];
                        bsum[j] += g;
                        bsx[j] = fmaf(g, xh, bsx[j]);
                    }
                }
            }
        }
        if (do_bn) {
            // reduce over the ROWS_PER_PASS rsub groups sharing each csub
            __syncthreads();                  // stage reads done; reuse LDS
            float* red = reinterpret_cast<float*>(stageA);  // [rsub][TBN][2]
            #pragma unroll
            for (int j = 0; j < 8; ++j) {
                red[(rsub * TBN + csub + j) * 2] = bsum[j];
                red[(rsub * TBN + csub + j) * 2 + 1] = bsx[j];
            }
            __syncthreads();
            const int gridM = gridDim.x;
            for (int cl = tid; cl < TBN; cl += 256) {
                float a = 0.f, b2 = 0.f;
                #pragma unroll 4
                for (int w = 0; w < ROWS_PER_PASS; ++w) {
                    a += red[(w * TBN + cl) * 2];
                    b2 += red[(w * TBN + cl) * 2 + 1];
                }
                int col = n0 + cl;
                if (col < Nout) {
                    bn.slab[(long)col * gridM + blockIdx.x] = a;
                    bn.slab[(long)Nout * gridM + (long)col * gridM
                            + blockIdx.x] = b2;
                }
            }
        }
    }

    if (MODE == 0 && stats) {
        // Per-channel partial sum/sumsq of this block's 128 output rows —
        // feeds the BN that consumes this conv (its stats pass never
        // re-reads y).  slab layout matches k_bn_combine: [2][Nout][gridM].
        __syncthreads();                       // done reading lds tiles
        float* red = reinterpret_cast<float*>(&lds_a[0][0][0]);  // [WAVES_M][TBN][2]
        #pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            float a = psum[ni], b = psq[ni];
            a += __shfl_down(a, 32, 64);
            a += __shfl_down(a, 16, 64);
            b += __shfl_down(b, 32, 64);
            b += __shfl_down(b, 16, 64);
            if ((lane & 48) == 0) {            // lanes 0..15 hold the totals
                int cl = wc * WN + ni * 16 + (lane & 15);
                red[(wr * TBN + cl) * 2] = a;
                red[(wr * TBN + cl) * 2 + 1] = b;
            }
        }
        __syncthreads();
        const int gridM = gridDim.x;
        for (int cl = tid; cl < TBN; cl += 256) {
            float a = 0.f, b = 0.f;
            #pragma unroll
            for (int w = 0; w < WAVES_M; ++w) {
                a += red[(w * TBN + cl) * 2];
                b += red[(w * TBN + cl) * 2 + 1];
            }
            int col = n0 + cl;
            if (col < Nout) {
                stats[(long)col * gridM + blockIdx.x] = a;
                stats[(long)Nout * gridM + (long)col * gridM + blockIdx.x] = b;
            }
        }
    }
}

template <int MODE, int TBN, int WAVES_M, int WAVES_N, bool STRIDE1 = true,
          int CBM_T = CBM, bool TAPS = false, bool WALK = false>
// min-4-waves/SIMD bound: the allocator packs the body into 122 arch
// VGPRs (no AGPRs, zero spills) instead of 84V+64A, lifting residency
// 3 -> 4 blocks/CU on the 128-wide tiles (and 4 -> 5 on the 64-wide) —
// these gather-fed GEMMs live on block-level parallelism.
__global__ __launch_bounds__(256, 4)
void k_conv_gemm(const bf16* __restrict__ Asrc, const bf16* __restrict__ Bsrc,
                 const float* __restrict__ bias, bf16* __restrict__ out,
                 ConvShape cs, int M, int Kgemm, int Nout,
                 float* __restrict__ stats = nullptr,
                 BnFuse bn = BnFuse{},
                 const bf16* __restrict__ addin = nullptr) {
    conv_gemm_body<MODE, TBN, WAVES_M, WAVES_N, STRIDE1, CBM_T, TAPS, WALK>(
        Asrc, Bsrc, bias, out, cs, M, Kgemm, Nout, stats, bn, addin);
}


// MODE-2 strided dgrad, all residue classes in ONE launch: blockIdx.z
// selects the class (its own ConvShape/M/Kgemm from the by-value pack).
// Class grids differ by at most one tile row, so grid.x is the max tile
// count and overhanging blocks exit before touching LDS (block-uniform).
struct ClsPack {
    ConvShape cs[4];
    int M[4];
    int K[4];
};

template <int TBN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(256, 4)
void k_conv_gemm_cls(const bf16* __restrict__ Asrc,
                     const bf16* __restrict__ Bsrc, bf16* __restrict__ out,
                     ClsPack pack, int Nout) {
    const int z = blockIdx.z;
    const int M = pack.M[z];
    if ((int)blockIdx.x * CBM >= M) return;
    conv_gemm_body<2, TBN, WAVES_M, WAVES_N, true, CBM>(
        Asrc, Bsrc, nullptr, out, pack.cs[z], M, pack.K[z], Nout,
        nullptr, BnFuse{}, nullptr);
}

// conv with Cin < 8 (e.g. the MNIST stem, Cin=1): direct VALU kernel,
// weights staged in LDS, thread computes 8 output channels of one (n,p,q).
__global__ void k_conv_small_cin(const bf16* __restrict__ x,
                                 const bf16* __restrict__ w,
                                 const float* __restrict__ bias,
                                 bf16* __restrict__ y, ConvShape cs, long M) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* wlds = reinterpret_cast<bf16*>(smem);   // [Ko][R*S*C]
    int rsc = cs.R * cs.S * cs.C;
    for (int i = threadIdx.x; i < cs.Ko * rsc; i += blockDim.x)
        wlds[i] = w[i];
    __syncthreads();
    long total = M * (cs.Ko / 8);
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long gstride = (long)gridDim.x * blockDim.x;
    for (; i < total; i += gstride) {
        int ko8 = (i % (cs.Ko / 8)) * 8;
        long gm = i / (cs.Ko / 8);
        int q = gm % cs.Q; long rem = gm / cs.Q;
        int p = rem % cs.P; int n = rem / cs.P;
        float acc[8] = {};
        for (int r = 0; r < cs.R; ++r) {
            int h = p * cs.stride + r - cs.pad;
            if (h < 0 || h >= cs.H) continue;
            for (int s = 0; s < cs.S; ++s) {
                int wc = q * cs.stride + s - cs.pad;
                if (wc < 0 || wc >= cs.W) continue;
                for (int c = 0; c < cs.C; ++c) {
                    float xv = bf2f(x[(((long)n * cs.H + h) * cs.W + wc) * cs.C + c]);
                    int kidx = (r * cs.S + s) * cs.C + c;
                    #pragma unroll
                    for (int j = 0; j < 8; ++j)
                        acc[j] = fmaf(xv, bf2f(wlds[(ko8 + j) * rsc + kidx]), acc[j]);
                }
            }
        }
        bf16x8_t o;
        #pragma unroll
        for (int j = 0; j < 8; ++j)
            o[j] = (short)f2us(acc[j] + (bias ? bias[ko8 + j] : 0.f));
        *reinterpret_cast<bf16x8_t*>(&y[gm * cs.Ko + ko8]) = o;
    }
}

// -------------------------------------------------------- backward weight ---

// Every MFMA leaf writes slab[s][ko, rsc] = Σ_{m in split s} dy[m][ko] ·
// im2col(x)[m][rsc] on a (ko tiles, rsc tiles, S) grid; split s owns the
// contraction steps s, s + S, ... of the leaf's DEPTH.  The operands are
// m-major in memory and the MFMA wants m contiguous per lane, so the leaves
// differ in how they transpose: packed pair stores (sb_pair, wide_pair) or
// LDS-DMA plus transposed reads (wide_dma).  plan_wgrad (hosts, below) picks
// the leaf and S.
constexpr int WBM = 64, WBN = 64;   // sb_pair tile; the wide leaves use 128

// combine slab -> dw fp32 in torch KCRS layout (fixed order, deterministic).
// BIAS: the slab carries S x Ko bias partials behind the S dw slices (see
// k_conv_wgrad_wide_pair) and the launch has one block more: the last block
// sums those into db while the others do dw (as a second grid-stride trip
// of the dw blocks the bias sums measured +6 us on conv2's combine).
template <bool BIAS = false>
__global__ void k_wgrad_combine(const float* __restrict__ slab, int S,
                                ConvShape cs, int Kgemm,
                                float* __restrict__ dw,
                                float* __restrict__ db) {
    long total = (long)cs.Ko * Kgemm;
    const int nb = BIAS ? gridDim.x - 1 : gridDim.x;
    if (BIAS && (int)blockIdx.x == nb) {
        const float* bs = slab + (long)S * total;
        for (int ko = threadIdx.x; ko < cs.Ko; ko += blockDim.x) {
            float v = 0.f;
            for (int s = 0; s < S; ++s) v += bs[(long)s * cs.Ko + ko];
            db[ko] = v;
        }
        return;
    }
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long stride = (long)nb * blockDim.x;
    int RS = cs.R * cs.S;
    for (; i < total; i += stride) {
        float v = 0.f;
        for (int s = 0; s < S; ++s) v += slab[(long)s * total + i];
        int ko = i / Kgemm;
        int rc = i % Kgemm;
        int c = rc % cs.C, rs = rc / cs.C;
        dw[((long)ko * cs.C + c) * RS + rs] = v;
    }
}

// Stage-1 combine for deep splits: sum CH consecutive s-slices per
// (chunk, i) into slab2[chunk][i] — identity layout, fixed order
// (deterministic).  Two passes beat one when S is deep: the single-pass
// combine is latency-bound (e.g. conv2's S=128 slab gives only 288
// blocks, each thread chewing 128 dependent 294-KB-strided loads —
// measured 40.7 us avg where ~38 MB of reads should take <6); this pass
// runs chunks× more waves and leaves the final KCRS scatter a shallow
// S/CH-deep sum.  BIAS: indices past ``total`` do the same for the Ko-wide
// bias partials, which sit behind the dw slices in both slabs.
template <bool BIAS = false>
__global__ void k_wgrad_combine_stage(const float* __restrict__ slab, int S,
                                      int CH, long total, int Ko,
                                      float* __restrict__ slab2) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (BIAS ? total + Ko : total)) return;
    const int c0 = blockIdx.y * CH;
    const int ce = min(S, c0 + CH);
    long ld = total;
    if (BIAS && i >= total) {
        slab += (long)S * total - total;            // -> bias partials
        slab2 += (long)gridDim.y * total - total;
        ld = Ko;
    }
    // two independent accumulator chains (fixed even/odd order — still
    // deterministic) so two loads are in flight per iteration
    float v0 = 0.f, v1 = 0.f;
    int s = c0;
    for (; s + 1 < ce; s += 2) {
        v0 += slab[(long)s * ld + i];
        v1 += slab[(long)(s + 1) * ld + i];
    }
    if (s < ce) v0 += slab[(long)s * ld + i];
    slab2[(long)blockIdx.y * ld + i] = v0 + v1;
}

// Pair-m single-buffer 64x64 wgrad: thread halves split the two operands;
// each thread stages m-PAIRs with packed b32 stores (conflict-free).
// DEPTH = staged contraction (32 or 64; 64 halves the barrier rate).
template <int DEPTH>
__global__ __launch_bounds__(256)
void k_conv_wgrad_sb_pair(const bf16* __restrict__ dy,
                          const bf16* __restrict__ x,
                          float* __restrict__ slab, ConvShape cs, long M,
                          int Kgemm, int S) {
    __shared__ bf16 lds_a[WBM][DEPTH + 8];   // [ko][m]
    __shared__ bf16 lds_b[WBN][DEPTH + 8];   // [rsc][m]
    constexpr int SLD = DEPTH + 8;
    constexpr int PAIRS = DEPTH / 2;         // m-pairs per row
    const int ko0 = blockIdx.x * WBM;
    const int rc0 = blockIdx.y * WBN;
    const int split = blockIdx.z;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6, wr = wid >> 1, wc = wid & 1;

    f32x4 acc[2][2] = {};
    const int m2 = (tid & (PAIRS - 1)) * 2;
    const int jsel = tid / PAIRS;            // 256/PAIRS j-slots
    constexpr int JSLOTS = 256 / PAIRS;      // 16 (D32) or 8 (D64)
    const bool is_b = jsel >= JSLOTS / 2;    // thread half stages A or B
    const int jb = (jsel % (JSLOTS / 2)) * 8;
    constexpr int JSTEP = (JSLOTS / 2) * 8;  // j covered per pass

    const long m_begin = (long)split * DEPTH;
    for (long mt = m_begin; mt < M; mt += (long)S * DEPTH) {
        long gm0 = mt + m2;
        const bool v0 = gm0 < M, v1 = gm0 + 1 < M;
        // decode once per m-pair (B threads only need it)
        unsigned q0 = 0, p0 = 0, n0_ = 0, q1 = 0, p1 = 0, n1_ = 0;
        if (is_b) {
            if (v0) {
                unsigned rem = fd_div((unsigned)gm0, cs.fdQ);
                q0 = fd_mod((unsigned)gm0, cs.fdQ, rem);
                n0_ = fd_div(rem, cs.fdP);
                p0 = fd_mod(rem, cs.fdP, n0_);
            }
            if (v1) {
                unsigned rem = fd_div((unsigned)gm0 + 1, cs.fdQ);
                q1 = fd_mod((unsigned)gm0 + 1, cs.fdQ, rem);
                n1_ = fd_div(rem, cs.fdP);
                p1 = fd_mod(rem, cs.fdP, n1_);
            }
        }
        #pragma unroll
        for (int j8 = jb; j8 < 64; j8 += JSTEP) {
            bf16x8_t t0 = {}, t1 = {};
            if (!is_b) {
                if (ko0 + j8 < cs.Ko) {
                    if (v0) t0 = *reinterpret_cast<const bf16x8_t*>(
                        &dy[gm0 * cs.Ko + ko0 + j8]);
                    if (v1) t1 = *reinterpret_cast<const bf16x8_t*>(
                        &dy[(gm0 + 1) * cs.Ko + ko0 + j8]);
                }
            } else {
                int gk = rc0 + j8;
                if (gk < Kgemm) {
                    unsigned rs = fd_div(gk, cs.fdC);
                    int c = fd_mod(gk, cs.fdC, rs);
                    int r = fd_div(rs, cs.fdS);
                    int sx = fd_mod(rs, cs.fdS, r);
                    if (v0) {
                        int h = (int)p0 * cs.stride + r - cs.pad;
                        int wcol = (int)q0 * cs.stride + sx - cs.pad;
                        if (h >= 0 && h < cs.H && wcol >= 0 && wcol < cs.W)
                            t0 = *reinterpret_cast<const bf16x8_t*>(
                                &x[(((long)n0_ * cs.H + h) * cs.W + wcol) * cs.C + c]);
                    }
                    if (v1) {
                        int h = (int)p1 * cs.stride + r - cs.pad;
                        int wcol = (int)q1 * cs.stride + sx - cs.pad;
                        if (h >= 0 && h < cs.H && wcol >= 0 && wcol < cs.W)
                            t1 = *reinterpret_cast<const bf16x8_t*>(
                                &x[(((long)n1_ * cs.H + h) * cs.W + wcol) * cs.C + c]);
                    }
                }
            }
            bf16* dst = is_b ? &lds_b[0][0] : &lds_a[0][0];
            #pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                unsigned pk = (unsigned)(unsigned short)t0[jj]
                    | ((unsigned)(unsigned short)t1[jj] << 16);
                const int row = j8 + jj;
                const int mph = m2 ^ ((row & 3) << 3);   // 8-block swizzle
                *reinterpret_cast<unsigned*>(&dst[row * SLD + mph]) = pk;
            }
        }
        __syncthreads();

        #pragma unroll
        for (int ks = 0; ks < DEPTH; ks += 32) {
            bf16x8_t af[2], bfr[2];
            const int kcol = ks + (lane >> 4) * 8;
            #pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int row = wr * 32 + mi * 16 + (lane & 15);
                af[mi] = *reinterpret_cast<const bf16x8_t*>(
                    &lds_a[row][kcol ^ ((row & 3) << 3)]);
            }
            #pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int row = wc * 32 + ni * 16 + (lane & 15);
                bfr[ni] = *reinterpret_cast<const bf16x8_t*>(
                    &lds_b[row][kcol ^ ((row & 3) << 3)]);
            }
            #pragma unroll
            for (int mi = 0; mi < 2; ++mi)
                #pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[mi], bfr[ni], acc[mi][ni], 0, 0, 0);
        }
        __syncthreads();
    }

    #pragma unroll
    for (int mi = 0; mi < 2; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            int col = rc0 + wc * 32 + ni * 16 + (lane & 15);
            if (col >= Kgemm) continue;
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                int row = ko0 + wr * 32 + mi * 16 + (lane >> 4) * 4 + r;
                if (row >= cs.Ko) continue;
                slab[((long)split * cs.Ko + row) * Kgemm + col] =
                    acc[mi][ni][r];
            }
        }
}

// Pair-m wide wgrad: 128(ko) x 128(rsc) tile, DEPTH-deep contraction (needs
// Ko >= 128 and Kgemm >= 128).  Each thread stages TWO consecutive m's per
// j-group so LDS writes are packed b32 (16 stores/operand/iter vs 32
// conflicted b16) — the stage phase of this tile is store-issue bound.
// wide_dma replaced it in the automatic dispatch; it stays as that leaf's
// bit-identity oracle (DDPX_WGRAD_V=wp / wq).
//
// BIAS: the blockIdx.y == 0 blocks (one per (ko tile, split)) also sum the
// staged dy tile along m straight from lds_a — two threads per ko row, one
// physical half-row each (a whole-row sum does not care about the XOR
// swizzle, and tail rows / tail m's are staged as zeros) — and write one
// bias partial per (split, ko) behind the dw slab, at slab + S*Ko*Kgemm,
// where the combine kernels pick it up.  The conv's bias gradient then
// costs no extra pass over dy.  BIAS=false compiles to the kernel it was.
template <int DEPTH = 64, bool BIAS = false>
__global__ // NOTE: a 4-waves/SIMD bound (V 78+64A -> 128+0A, occ 3->4) was tried
// here like k_conv_gemm's and REVERTED: measured 285.7 vs 263.1 us —
// this kernel's pair-store stage phase wants the AGPR split, not
// residency (same lesson as the depth-64 staging dead ends).
__launch_bounds__(256)
void k_conv_wgrad_wide_pair(const bf16* __restrict__ dy,
                            const bf16* __restrict__ x,
                            float* __restrict__ slab, ConvShape cs, long M,
                            int Kgemm, int S) {
    // row stride DEPTH+24: PMC showed 2.8-4.6k LDS-conflict stall cycles
    // per wave at +8 padding; +24 keeps the 16-lane b128 fragment reads
    // bank-disjoint (stride 44/28 dwords, gcd 4, all 16 starts distinct)
    // NOTE: row-stride padding (+8 → +24) measured ZERO effect on the
    // LDS conflict counter (2848/4608 cycles/wave both ways) — the
    // conflicts are between the (lane>>4) k-sub-groups of the b128
    // fragment reads, which a row-stride change cannot separate.  The
    // XOR 8-block swizzle below (phys m-block = m ^ ((row&3)<<3), same
    // idiom as the fwd glds swizzle) is the fix that addresses it.
    constexpr int SLD = DEPTH + 8;
    __shared__ bf16 lds_a[128][SLD];
    __shared__ bf16 lds_b[128][SLD];
    const int ko0 = blockIdx.x * 128;
    const int rc0 = blockIdx.y * 128;
    const int split = blockIdx.z;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6, wr = wid >> 1, wc = wid & 1;

    f32x4 acc[4][4] = {};
    [[maybe_unused]] float bsum = 0.f;
    const int m2 = (tid & (DEPTH / 2 - 1)) * 2;   // m, m+1
    const int jb = (tid / (DEPTH / 2)) * 8;
    constexpr int JSTEP2 = (256 / (DEPTH / 2)) * 8;  // j per pass
    const long m_begin = (long)split * DEPTH;

    for (long mt = m_begin; mt < M; mt += (long)S * DEPTH) {
        long gm0 = mt + m2;
        const bool v0 = gm0 < M, v1 = gm0 + 1 < M;
        // decode both m's once (x gather bases)
        unsigned q0 = 0, p0 = 0, n0_ = 0, q1 = 0, p1 = 0, n1_ = 0;
        if (v0) {
            unsigned rem = fd_div((unsigned)gm0, cs.fdQ);
            q0 = fd_mod((unsigned)gm0, cs.fdQ, rem);
            n0_ = fd_div(rem, cs.fdP);
            p0 = fd_mod(rem, cs.fdP, n0_);
        }
        if (v1) {
            unsigned rem = fd_div((unsigned)gm0 + 1, cs.fdQ);
            q1 = fd_mod((unsigned)gm0 + 1, cs.fdQ, rem);
            n1_ = fd_div(rem, cs.fdP);
            p1 = fd_mod(rem, cs.fdP, n1_);
        }
        #pragma unroll
        for (int j = jb; j < 128; j += JSTEP2) {
            bf16x8_t a0 = {}, a1 = {};
            if (ko0 + j < cs.Ko) {
                if (v0) a0 = *reinterpret_cast<const bf16x8_t*>(
                    &dy[gm0 * cs.Ko + ko0 + j]);
                if (v1) a1 = *reinterpret_cast<const bf16x8_t*>(
                    &dy[(gm0 + 1) * cs.Ko + ko0 + j]);
            }
            bf16x8_t b0 = {}, b1 = {};
            int gk = rc0 + j;
            if (gk < Kgemm) {
                unsigned rs = fd_div(gk, cs.fdC);
                int c = fd_mod(gk, cs.fdC, rs);
                int r = fd_div(rs, cs.fdS);
                int sx = fd_mod(rs, cs.fdS, r);
                if (v0) {
                    int h = (int)p0 * cs.stride + r - cs.pad;
                    int wcol = (int)q0 * cs.stride + sx - cs.pad;
                    if (h >= 0 && h < cs.H && wcol >= 0 && wcol < cs.W)
                        b0 = *reinterpret_cast<const bf16x8_t*>(
                            &x[(((long)n0_ * cs.H + h) * cs.W + wcol) * cs.C + c]);
                }
                if (v1) {
                    int h = (int)p1 * cs.stride + r - cs.pad;
                    int wcol = (int)q1 * cs.stride + sx - cs.pad;
                    if (h >= 0 && h < cs.H && wcol >= 0 && wcol < cs.W)
                        b1 = *reinterpret_cast<const bf16x8_t*>(
                            &x[(((long)n1_ * cs.H + h) * cs.W + wcol) * cs.C + c]);
                }
            }
            #pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                unsigned pa = (unsigned)(unsigned short)a0[jj]
                    | ((unsigned)(unsigned short)a1[jj] << 16);
                unsigned pb = (unsigned)(unsigned short)b0[jj]
                    | ((unsigned)(unsigned short)b1[jj] << 16);
                const int row = j + jj;
                const int mph = m2 ^ ((row & 3) << 3);   // 8-block swizzle
                *reinterpret_cast<unsigned*>(&lds_a[row][mph]) = pa;
                *reinterpret_cast<unsigned*>(&lds_b[row][mph]) = pb;
            }
        }
        __syncthreads();

        if constexpr (BIAS) {
            if (blockIdx.y == 0) {
                const bf16* rp = &lds_a[tid >> 1][(tid & 1) * (DEPTH / 2)];
                #pragma unroll
                for (int i = 0; i < DEPTH / 2; i += 8) {
                    bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(rp + i);
                    #pragma unroll
                    for (int jj = 0; jj < 8; ++jj)
                        bsum += us2f((unsigned short)v[jj]);
                }
            }
        }

        #pragma unroll
        for (int ks = 0; ks < DEPTH; ks += 32) {
            bf16x8_t af[4], bfr[4];
            const int kcol = ks + (lane >> 4) * 8;
            #pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int row = wr * 64 + mi * 16 + (lane & 15);
                af[mi] = *reinterpret_cast<const bf16x8_t*>(
                    &lds_a[row][kcol ^ ((row & 3) << 3)]);
            }
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int row = wc * 64 + ni * 16 + (lane & 15);
                bfr[ni] = *reinterpret_cast<const bf16x8_t*>(
                    &lds_b[row][kcol ^ ((row & 3) << 3)]);
            }
            #pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                #pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[mi], bfr[ni], acc[mi][ni], 0, 0, 0);
        }
        __syncthreads();
    }

    #pragma unroll
    for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            int col = rc0 + wc * 64 + ni * 16 + (lane & 15);
            if (col >= Kgemm) continue;
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                int row = ko0 + wr * 64 + mi * 16 + (lane >> 4) * 4 + r;
                if (row >= cs.Ko) continue;
                slab[((long)split * cs.Ko + row) * Kgemm + col] =
                    acc[mi][ni][r];
            }
        }

    if constexpr (BIAS) {
        if (blockIdx.y == 0) {
            bsum += __shfl_xor(bsum, 1, 64);   // the row's other half
            const int row = ko0 + (tid >> 1);
            if (!(tid & 1) && row < cs.Ko)
                slab[(long)S * cs.Ko * Kgemm + (long)split * cs.Ko + row] =
                    bsum;
        }
    }
}

// fd_div as a select, not a branch: keeps wide_dma's per-tile address block
// one straight run of VALU the scheduler can place under the DMA wait
DEV_INLINE unsigned fd_div_sel(unsigned n, FastDiv f) {
    unsigned hi = (unsigned)(((unsigned long long)n * f.mul) >> 32);
    return (f.mul == 0 ? n : hi) >> f.shift;
}

typedef short tr16x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) tr16x4_t* lds_tr16_ptr;

// LDS-DMA staged wide wgrad: k_conv_wgrad_wide_pair's grid, slab layout,
// split order, 2x2 waves of 64x64 and k->m mapping, but the forward kernel's
// staging.  Both operands are m-major in memory, so 16 B global_load_lds
// fills NATURAL images img_a[m][ko] / img_b[m][rsc] (no VGPR round trip, no
// pack VALU, no ds_write) and the MFMA fragments (m contiguous per lane) come
// from gfx950's transposed read ds_read_b64_tr_b16: within a 16-lane group,
// lane g addresses img[M0 + (g>>2)][col + (g&3)*4] and receives
// img[M0 + j][col + g], j = 0..3 (tools/microtests/tr16_probe.hip); a
// fragment is two reads 4 rows apart.  The instruction needs EXEC all ones:
// nothing lane-divergent encloses the read + MFMA block.
//
// Rows are 256 B, so every row starts on bank 0.  The 32 lanes of one read
// service group touch rows M0+{0..3} and M0+8+{0..3}, 32 B each; the 16 B
// segments are XOR-swizzled with 2*((row&3) | ((row>>3)&1)<<2), which puts
// those eight 32 B pieces on eight disjoint bank octets.  glds writes
// lane-linear, so the swizzle sits on the per-lane SOURCE address and is
// repeated on the reads (rule 21, as conv_gemm_body).  The value is the same
// for row and row+4 (the second half-fragment is an immediate offset) and,
// for the staging lanes, the same for every chunk a lane fills: a lane's
// logical segment never changes, so its (ko) and (r, s, c) decode runs once.
// Out-of-range lanes (m >= M, ko >= Ko, rsc >= Kgemm, padding taps) read
// g_zero16; no lane hands the DMA an address outside dy or x.
//
// Same split, depth, zero fills and MFMA order as wide_pair, so dw is
// bit-identical to that leaf.  BIAS: blockIdx.y == 0 blocks sum img_a along
// m with eight accumulators per ko, DEPTH/8 rows of every tile each, joined
// serially at the end: a chain of tiles*DEPTH/8 + 7 additions, inside the
// tiles*DEPTH/2 + 1 that the bound in tests/test_gpu_wgrad_bias.py assumes.
//
// Register bound: 3 blocks/CU measured best.  Left free, the compiler
// splits 64 accumulators into AGPRs and DEPTH 64 lands at 2 waves/SIMD
// (114+64A): conv3 122.6 vs 111.1 us, conv4 254.3 vs 221.9.  DEPTH 32 ties
// with the bound free (conv2 217.7 vs 216.2).  Only DEPTH 64 computes the
// next tile's addresses ahead (AHEAD): DEPTH 32 under a 4-block bound
// spilled with it, and was not tried again at 3.
template <int DEPTH = 64, bool BIAS = false>
__global__ __launch_bounds__(256, 3)
void k_conv_wgrad_wide_dma(const bf16* __restrict__ dy,
                           const bf16* __restrict__ x,
                           float* __restrict__ slab, ConvShape cs, long M,
                           int Kgemm, int S) {
    __shared__ __align__(16) bf16 img_a[DEPTH][128];   // [m][ko]
    __shared__ __align__(16) bf16 img_b[DEPTH][128];   // [m][rsc]
    constexpr int NCH = DEPTH / 16;   // 4-row glds chunks per wave per image
    constexpr bool AHEAD = DEPTH == 64;
    const int ko0 = blockIdx.x * 128;
    const int rc0 = blockIdx.y * 128;
    const int split = blockIdx.z;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6, wr = wid >> 1, wc = wid & 1;

    // ---- staging: wave wid fills chunks wid + 4i, rows 4*chunk + srow ----
    const int srow = lane >> 4;
    const int lseg = (lane & 15) ^ (2 * (srow | (((wid >> 1) & 1) << 2)));
    const int a_ko = ko0 + lseg * 8;
    const bool a_ok = a_ko < cs.Ko;
    const int b_gk = rc0 + lseg * 8;
    const bool b_ok = b_gk < Kgemm;
    int b_c = 0, b_dh = 0, b_dw = 0;
    if (b_ok) {
        unsigned rs = fd_div(b_gk, cs.fdC);
        b_c = fd_mod(b_gk, cs.fdC, rs);
        unsigned r = fd_div(rs, cs.fdS);
        b_dw = (int)fd_mod(rs, cs.fdS, r) - cs.pad;
        b_dh = (int)r - cs.pad;
    }
    const bf16* const zsrc = reinterpret_cast<const bf16*>(g_zero16);
    const bf16* sa[NCH];
    const bf16* sb[NCH];
    auto sources = [&](long mt) {
        #pragma unroll
        for (int i = 0; i < NCH; ++i) {
            // branch-free: index arithmetic on an out-of-range row is
            // harmless, only the final select decides what is dereferenced
            const long gm = mt + (wid + 4 * i) * 4 + srow;
            const bool m_ok = gm < M;
            unsigned rem = fd_div_sel((unsigned)gm, cs.fdQ);
            int q = fd_mod((unsigned)gm, cs.fdQ, rem);
            unsigned n = fd_div_sel(rem, cs.fdP);
            int p = fd_mod(rem, cs.fdP, n);
            int h = p * cs.stride + b_dh;
            int wcol = q * cs.stride + b_dw;
            const bool x_ok = m_ok & b_ok & (h >= 0) & (h < cs.H) &
                              (wcol >= 0) & (wcol < cs.W);
            const long oa = gm * cs.Ko + a_ko;
            const long ob = (((long)n * cs.H + h) * cs.W + wcol) * cs.C + b_c;
            sa[i] = (m_ok & a_ok) ? dy + oa : zsrc;
            sb[i] = x_ok ? x + ob : zsrc;
        }
    };

    // ---- fragment reads: element offsets, constant over tiles ----
    const int g = lane & 15;
    const int rsw = 2 * ((g >> 2) | (((lane >> 4) & 1) << 2));
    const int rbase = ((lane >> 4) * 8 + (g >> 2)) * 128 + (g & 1) * 4;
    const int rseg = (g & 3) >> 1;
    int offa[4], offb[4];
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
        offa[i] = rbase + ((wr * 8 + i * 2 + rseg) ^ rsw) * 8;
        offb[i] = rbase + ((wc * 8 + i * 2 + rseg) ^ rsw) * 8;
    }
    auto frag = [](const bf16* p) {
        tr16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_tr16_ptr)p);
        tr16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_tr16_ptr)(p + 4 * 128));
        return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    };

    f32x4 acc[4][4] = {};
    [[maybe_unused]] float bsum[4] = {};
    const long m_begin = (long)split * DEPTH;
    const long m_step = (long)S * DEPTH;
    if (AHEAD && m_begin < M) sources(m_begin);

    for (long mt = m_begin; mt < M; mt += m_step) {
        if (!AHEAD) sources(mt);
        #pragma unroll
        for (int i = 0; i < NCH; ++i) {
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) unsigned short*)sa[i],
                (__attribute__((address_space(3))) unsigned short*)
                    &img_a[(wid + 4 * i) * 4][0], 16, 0, 0);
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) unsigned short*)sb[i],
                (__attribute__((address_space(3))) unsigned short*)
                    &img_b[(wid + 4 * i) * 4][0], 16, 0, 0);
        }
        // next tile's addresses while this tile's DMA is in flight
        if (AHEAD && mt + m_step < M) sources(mt + m_step);
        __syncthreads();   // vmcnt(0) for the in-flight glds + barrier

        if constexpr (BIAS) {
            if (blockIdx.y == 0) {
                // thread = (row group tid>>5, ko quad tid&31): 8 B reads of
                // the group's DEPTH/8 rows (the swizzle moves whole 16 B
                // segments, so a quad stays contiguous)
                const int kq = tid & 31;
                const bf16* rp = &img_a[(tid >> 5) * (DEPTH / 8)][(kq & 1) * 4];
                #pragma unroll
                for (int i = 0; i < DEPTH / 8; ++i) {
                    // row = (tid>>5)*(DEPTH/8) + i: its swizzle bits
                    const int row = (tid >> 5) * (DEPTH / 8) + i;
                    const int sw = 2 * ((row & 3) | (((row >> 3) & 1) << 2));
                    s16x4 v = *reinterpret_cast<const s16x4*>(
                        rp + i * 128 + (((kq >> 1) ^ sw) << 3));
                    #pragma unroll
                    for (int jj = 0; jj < 4; ++jj)
                        bsum[jj] += us2f((unsigned short)v[jj]);
                }
            }
        }

        #pragma unroll
        for (int ks = 0; ks < DEPTH; ks += 32) {
            bf16x8_t af[4], bfr[4];
            #pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                af[mi] = frag(&img_a[ks][0] + offa[mi]);
            #pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                bfr[ni] = frag(&img_b[ks][0] + offb[ni]);
            #pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                #pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[mi], bfr[ni], acc[mi][ni], 0, 0, 0);
        }
        __syncthreads();
    }

    #pragma unroll
    for (int mi = 0; mi < 4; ++mi)
        #pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            int col = rc0 + wc * 64 + ni * 16 + (lane & 15);
            if (col >= Kgemm) continue;
            #pragma unroll
            for (int r = 0; r < 4; ++r) {
                int row = ko0 + wr * 64 + mi * 16 + (lane >> 4) * 4 + r;
                if (row >= cs.Ko) continue;
                slab[((long)split * cs.Ko + row) * Kgemm + col] =
                    acc[mi][ni][r];
            }
        }

    if constexpr (BIAS) {
        if (blockIdx.y == 0) {
            // join the two half-tile chains (the loop's last barrier has
            // retired every read of img_a)
            float* join = reinterpret_cast<float*>(&img_a[0][0]);  // [8][128]
            #pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                join[(tid >> 5) * 128 + (tid & 31) * 4 + jj] = bsum[jj];
            __syncthreads();
            const int row = ko0 + tid;
            if (tid < 128 && row < cs.Ko) {
                float s = join[tid];
                #pragma unroll
                for (int gi = 1; gi < 8; ++gi) s += join[gi * 128 + tid];
                slab[(long)S * cs.Ko * Kgemm + (long)split * cs.Ko + row] = s;
            }
        }
    }
}

// conv1 wgrad, fully specialized C==1 / 3x3 (the MNIST stem): each walker
// wave sweeps a CONTIGUOUS output range with incremental (n,p,q) tracking —
// no divisions in the inner loop — and a 3x3 sliding x-window in registers
// (q+1 reuses 6 of 9 taps).  dy loads are lane-coalesced along Ko; x loads
// are wave-uniform scalar broadcasts.  slab layout matches
// k_wgrad_small_rsc ([k][Ko][split]) so the combine kernel is shared.
// Since k_wgrad_c1_r3_stream (below) this is the fallback for what that
// kernel does not take: Ko % 8 != 0.
__global__ void k_wgrad_c1_r3(const bf16* __restrict__ dy,
                              const bf16* __restrict__ x,
                              float* __restrict__ slab, ConvShape cs,
                              long M, int S) {
    const int ko = threadIdx.x & 63;
    const int walker = threadIdx.x >> 6;          // 4 walker waves / block
    const long wslot = (long)blockIdx.x * 4 + walker;
    const long nslots = (long)S * 4;
    const long chunk = (M + nslots - 1) / nslots;
    long gm = wslot * chunk;
    const long gm_end = min(M, gm + chunk);
    float acc[9] = {};
    if (gm < gm_end && ko < cs.Ko) {
        int q = (int)(gm % cs.Q);
        long rem = gm / cs.Q;
        int p = (int)(rem % cs.P);
        int n = (int)(rem / cs.P);
        float xw[9];           // window: xw[r*3+s] = x[p*st+r-pad][q*st+s-pad]
        auto ld = [&](int h, int wc) -> float {
            return (h >= 0 && h < cs.H && wc >= 0 && wc < cs.W)
                ? bf2f(x[((long)n * cs.H + h) * cs.W + wc]) : 0.f;
        };
        auto fill = [&]() {
            #pragma unroll
            for (int r = 0; r < 3; ++r)
                #pragma unroll
                for (int s = 0; s < 3; ++s)
                    xw[r * 3 + s] = ld(p * cs.stride + r - cs.pad,
                                       q * cs.stride + s - cs.pad);
        };
        fill();
        // NOTE: an 8-deep dy load batch was tried and REVERTED (161.7 vs
        // 142.2 us measured): the per-row tail branches inside the
        // unrolled batch cost more than the extra loads-in-flight win —
        // the sequential 128 B/row stream already rides the L2 prefetch.
        bf16 gnext = dy[gm * cs.Ko + ko];
        for (;;) {
            float g = bf2f(gnext);
            if (gm + 1 < gm_end)               // prefetch next row's dy
                gnext = dy[(gm + 1) * cs.Ko + ko];
            #pragma unroll
            for (int k = 0; k < 9; ++k) acc[k] = fmaf(g, xw[k], acc[k]);
            if (++gm >= gm_end) break;
            if (++q == cs.Q) {
                q = 0;
                if (++p == cs.P) { p = 0; ++n; }
                fill();
            } else if (cs.stride == 1) {
                #pragma unroll
                for (int r = 0; r < 3; ++r) {
                    xw[r * 3] = xw[r * 3 + 1];
                    xw[r * 3 + 1] = xw[r * 3 + 2];
                    xw[r * 3 + 2] = ld(p + r - cs.pad, q + 2 - cs.pad);
                }
            } else {
                fill();
            }
        }
    }
    __shared__ float red[4][64];
    for (int k = 0; k < 9; ++k) {
        __syncthreads();
        red[walker][ko] = acc[k];
        __syncthreads();
        if (walker == 0 && ko < cs.Ko) {
            float t = red[0][ko] + red[1][ko] + red[2][ko] + red[3][ko];
            slab[((long)k * cs.Ko + ko) * gridDim.x + blockIdx.x] = t;
        }
    }
}

// Streaming stem wgrad (C == 1, 3x3, Ko % 8 == 0, Ko <= 64).  The walker
// above moves 128 B per wave instruction with two rows in flight and runs at
// a tenth of HBM rate; here every lane loads 16 B (8 channels) of dy, so
// one wave instruction covers RPL = 64 / (Ko/8) consecutive output rows
// (1 KiB at Ko = 64), and SU independent loads are issued per loop trip.
// Designed for >= 32 KiB of dy loads in flight per CU: 4 KiB per wave x 8
// resident waves; at the 3 blocks/CU the register count allows it is 48 KiB.
// Each lane decodes its own (n, p, q) with the magic divisors (rows of one
// load may wrap image rows and images) and reads its 3x3 x window with plain
// cached loads — x is L2-resident.  Per lane: 9 taps x 8 channels of fp32
// accumulators, plus (BIAS) the plain dy sums as a tenth "tap"; all indices
// are compile-time.  The end is fixed-order: per tap, the 256 threads park
// their 8 sums in LDS and thread c < Ko adds the 4 waves x RPL rows of
// channel c in index order, then writes slab[k][Ko][block] (the layout of
// k_wgrad_small_rsc, so its combine is shared; tap 9 is db).
constexpr int SU = 4;
template <bool BIAS, bool PADDED>
__global__ __launch_bounds__(256)
void k_wgrad_c1_r3_stream(const bf16* __restrict__ dy,
                          const bf16* __restrict__ x,
                          float* __restrict__ slab, ConvShape cs, long M,
                          long chunk) {
    constexpr int NT = BIAS ? 10 : 9;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int lpr = cs.Ko >> 3;            // lanes per dy row
    const int rpl = 64 / lpr;              // rows per wave load
    const int r_in = lane / lpr;
    const int cg = lane - r_in * lpr;
    const bool lane_on = r_in < rpl;
    const long w0 = ((long)blockIdx.x * 4 + wave) * chunk;
    const long w1 = min(M, w0 + chunk);
    const unsigned short* xs = reinterpret_cast<const unsigned short*>(x);
    float acc[NT][8] = {};
    for (long base = w0; base < w1; base += (long)rpl * SU) {
        bf16x8_t g[SU];
        long gmv[SU];
        #pragma unroll
        for (int u = 0; u < SU; ++u) {
            const long gm = base + u * rpl + r_in;
            const bool ok = lane_on && gm < w1;
            gmv[u] = ok ? gm : -1;
            // off lanes read row 0 (always there) and are zeroed below
            g[u] = *reinterpret_cast<const bf16x8_t*>(
                &dy[(ok ? gm : 0) * cs.Ko + cg * 8]);
        }
        #pragma unroll
        for (int u = 0; u < SU; ++u) {
            const bool ok = gmv[u] >= 0;
            const unsigned gm = ok ? (unsigned)gmv[u] : 0u;
            const unsigned rem = fd_div(gm, cs.fdQ);
            const int q = (int)fd_mod(gm, cs.fdQ, rem);
            const int n = (int)fd_div(rem, cs.fdP);
            const int p = (int)fd_mod(rem, cs.fdP, (unsigned)n);
            const int h0 = p * cs.stride - cs.pad;
            const int c0 = q * cs.stride - cs.pad;
            const long xb = ((long)n * cs.H + h0) * cs.W + c0;
            float xw[9];
            #pragma unroll
            for (int r = 0; r < 3; ++r)
                #pragma unroll
                for (int s = 0; s < 3; ++s) {
                    bool inb = true;
                    if (PADDED)
                        inb = h0 + r >= 0 && h0 + r < cs.H &&
                              c0 + s >= 0 && c0 + s < cs.W;
                    xw[r * 3 + s] = inb ? us2f(xs[xb + r * cs.W + s]) : 0.f;
                }
            #pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float gf = ok ? us2f((unsigned short)g[u][j]) : 0.f;
                #pragma unroll
                for (int k = 0; k < 9; ++k)
                    acc[k][j] = fmaf(gf, xw[k], acc[k][j]);
                if (BIAS) acc[NT - 1][j] += gf;
            }
        }
    }
    __shared__ float red[8][256 + 8];   // +8: reader banks rj*8 + rc distinct
    const int rc = tid >> 3, rj = tid & 7;   // reader: channel rc*8 + rj
    #pragma unroll
    for (int k = 0; k < NT; ++k) {
        __syncthreads();
        #pragma unroll
        for (int j = 0; j < 8; ++j) red[j][tid] = acc[k][j];
        __syncthreads();
        if (tid < cs.Ko) {
            float t = 0.f;
            for (int w = 0; w < 4; ++w)
                for (int r = 0; r < rpl; ++r)
                    t += red[rj][w * 64 + r * lpr + rc];
            slab[((long)k * cs.Ko + tid) * gridDim.x + blockIdx.x] = t;
        }
    }
}

// conv1-style wgrad fast path (RSC <= 16, Ko <= 64): ONE pass over dy per
// split — all RSC taps accumulate in registers; dy loads are lane-coalesced
// along Ko, x loads are wave-uniform broadcasts.
__global__ void k_wgrad_small_rsc(const bf16* __restrict__ dy,
                                  const bf16* __restrict__ x,
                                  float* __restrict__ slab, ConvShape cs,
                                  long M, int S, int RSC) {
    int ko = threadIdx.x & 63;
    int walker = threadIdx.x >> 6;    // 4 walkers
    int split = blockIdx.x;
    float acc[16] = {};
    for (long gm = (long)split * 4 + walker; gm < M; gm += (long)S * 4) {
        int q = gm % cs.Q; long rem = gm / cs.Q;
        int p = rem % cs.P; int n = rem / cs.P;
        float g = (ko < cs.Ko) ? bf2f(dy[gm * cs.Ko + ko]) : 0.f;
        #pragma unroll 1
        for (int k = 0; k < RSC; ++k) {
            int c = k % cs.C; int rs = k / cs.C;
            int r = rs / cs.S, s = rs % cs.S;
            int h = p * cs.stride + r - cs.pad;
            int wcol = q * cs.stride + s - cs.pad;
            float xv = (h >= 0 && h < cs.H && wcol >= 0 && wcol < cs.W)
                ? bf2f(x[(((long)n * cs.H + h) * cs.W + wcol) * cs.C + c])
                : 0.f;
            acc[k] = fmaf(g, xv, acc[k]);
        }
    }
    __shared__ float red[4][64];
    for (int k = 0; k < RSC; ++k) {
        __syncthreads();
        red[walker][ko] = acc[k];
        __syncthreads();
        if (walker == 0 && ko < cs.Ko) {
            float t = red[0][ko] + red[1][ko] + red[2][ko] + red[3][ko];
            // slab layout [RSC*Ko][S]: combine waves sweep the splits coalesced
            slab[((long)k * cs.Ko + ko) * gridDim.x + split] = t;
        }
    }
}

// combine for the fast small-RSC path: wave per (k, ko), lanes sweep S.
// With db set the slab has one more "tap", k == RSC: the bias partials.
__global__ void k_wgrad_small_rsc_combine(const float* __restrict__ slab,
                                          int S, ConvShape cs, int RSC,
                                          float* __restrict__ dw,
                                          float* __restrict__ db) {
    int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (i >= (RSC + (db != nullptr)) * cs.Ko) return;
    float v = 0.f;
    for (int s = lane; s < S; s += 64) v += slab[(long)i * S + s];
    v = wave_reduce_sum(v);
    if (lane) return;
    int ko = i % cs.Ko;
    int k = i / cs.Ko;
    if (k == RSC) { db[ko] = v; return; }
    int c = k % cs.C, rs = k / cs.C;
    dw[((long)ko * cs.C + c) * (cs.R * cs.S) + rs] = v;
}

// conv1-style wgrad (Cin < 8): per-(rs, split, ko-block) block, lanes along
// Ko — blockIdx.z walks Ko in 64-wide blocks so every output channel is
// covered (the combine reads all Ko columns of the slab)
__global__ void k_wgrad_small_cin(const bf16* __restrict__ dy,
                                  const bf16* __restrict__ x,
                                  float* __restrict__ slab, ConvShape cs,
                                  long M, int S) {
    int rsc = blockIdx.x;    // (r*S_ + s)*C + c  flattened small index
    int split = blockIdx.y;
    int c = rsc % cs.C, rsq = rsc / cs.C;
    int r = rsq / cs.S, s = rsq % cs.S;
    int kl = threadIdx.x & 63;
    int ko = blockIdx.z * 64 + kl;
    int walker = threadIdx.x >> 6;    // 4 walkers
    __shared__ float red[4][64];
    float acc = 0.f;
    if (ko < cs.Ko) {
        for (long gm = (long)split * 4 + walker; gm < M; gm += (long)S * 4) {
            int q = gm % cs.Q; long rem = gm / cs.Q;
            int p = rem % cs.P; int n = rem / cs.P;
            int h = p * cs.stride + r - cs.pad;
            int wcol = q * cs.stride + s - cs.pad;
            if (h < 0 || h >= cs.H || wcol < 0 || wcol >= cs.W) continue;
            float xv = bf2f(x[(((long)n * cs.H + h) * cs.W + wcol) * cs.C + c]);
            acc = fmaf(bf2f(dy[gm * cs.Ko + ko]), xv, acc);
        }
    }
    red[walker][kl] = acc;
    __syncthreads();
    if (walker == 0 && ko < cs.Ko) {
        float t = 0.f;
        #pragma unroll
        for (int w = 0; w < 4; ++w) t += red[w][kl];
        // slab layout [S][rsc_total][Ko]
        slab[((long)split * gridDim.x + rsc) * cs.Ko + ko] = t;
    }
}

__global__ void k_wgrad_small_combine(const float* __restrict__ slab, int S,
                                      ConvShape cs, int rsc_total,
                                      float* __restrict__ dw) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rsc_total * cs.Ko) return;
    int ko = i % cs.Ko;
    int rc = i / cs.Ko;
    float v = 0.f;
    for (int s = 0; s < S; ++s)
        v += slab[((long)s * rsc_total + rc) * cs.Ko + ko];
    int c = rc % cs.C, rs = rc / cs.C;
    dw[((long)ko * cs.C + c) * (cs.R * cs.S) + rs] = v;
}

// ------------------------------------------------------------------ hosts ---

static ConvShape make_shape(int N, int C, int H, int W, int Ko, int R, int S,
                            int stride, int pad) {
    ConvShape cs;
    cs.N = N; cs.C = C; cs.H = H; cs.W = W;
    cs.Ko = Ko; cs.R = R; cs.S = S; cs.stride = stride; cs.pad = pad;
    cs.P = (cs.H + 2 * pad - R) / stride + 1;
    cs.Q = (cs.W + 2 * pad - S) / stride + 1;
    init_fastdiv(cs);
    return cs;
}

static ConvShape make_shape(const at::Tensor& x, int Ko, int R, int S,
                            int stride, int pad) {
    return make_shape(x.size(0), x.size(1), x.size(2), x.size(3), Ko, R, S,
                      stride, pad);
}

static at::Tensor empty_nhwc(const at::Tensor& like, long n, long c, long h,
                             long w) {
    return at::empty({n, c, h, w},
                     like.options().memory_format(at::MemoryFormat::ChannelsLast));
}

// K loop of k_conv_gemm: "walk" (scalar tap walk, the WALK instantiations)
// or "decode" (per-chunk address decode).  The one place that decides; pure
// host arithmetic.  kwalk: -1 automatic, 0 decode, 1 forces walk; a forced
// walk on a shape it does not fit runs decode, and the plan says so.  Walk
// fits MODE 0 with C % CBK == 0 and stride-1 MODE 1 with Ko % CBK == 0 (a
// K-tile inside one tap); the kernel's tap offset is an int, its per-lane
// offsets are 64-bit.
static const char* plan_kloop(int mode, const ConvShape& cs, long kwalk) {
    TORCH_CHECK(kwalk >= -1 && kwalk <= 1, "conv kwalk must be -1 "
                "(automatic), 0 (decode) or 1 (walk); got ", kwalk);
    bool fits = false;
    // the tap offset the kernel forms, (r*W + s)*C + c0 with r < R, s < S
    // (Q and Ko for dgrad), must fit its int
    if (mode == 0)
        fits = cs.C % CBK == 0 &&
               ((long)cs.R * cs.W + cs.S) * cs.C < INT_MAX;
    else if (mode == 1)
        fits = cs.stride == 1 && cs.Ko % CBK == 0 &&
               ((long)cs.R * cs.Q + cs.S) * cs.Ko < INT_MAX;
    if (!fits || kwalk == 0) return "decode";
    // Automatic is the fit rule: the walk loop runs a subset of the decode
    // loop's instructions on the same data in the same order, so there is no
    // shape-dependent trade, and no class measured was slower (every one is
    // 20-30 % faster by its median: tools/bench_kernels.py --kwalk,
    // docs/KERNELS.md).
    return "walk";
}

// The one tile choice of forward and dgrad: a 128-channel output tile on
// 2x2 waves from 128 output channels up, else (or with narrow) 64 channels
// on 4x1 waves.
// NOTE: a 256-row tile for the narrow (< 128 channels) case was tried and
// REVERTED — its 40 KB LDS drops residency 6 -> 4 blocks/CU and measured
// 20-45% slower (same lesson as the 2-buf glds ring: this kernel lives on
// block-level parallelism).
template <int MODE, bool STRIDE1 = true>
static void launch_conv_gemm(hipStream_t stream, int grid_m, int n_channels,
                             bool narrow, const bf16* Asrc, const bf16* Bsrc,
                             const float* bias, bf16* out,
                             const ConvShape& cs, long M, int Kgemm,
                             float* stats, BnFuse bn, const bf16* addin,
                             long kwalk = 0) {
    if constexpr (MODE != 2) {
        if (plan_kloop(MODE, cs, kwalk)[0] == 'w') {
            if (n_channels >= 128 && !narrow)
                hipLaunchKernelGGL(
                    (k_conv_gemm<MODE, 128, 2, 2, STRIDE1, CBM, false, true>),
                    dim3(grid_m, ceil_div_i(n_channels, 128)), dim3(256), 0,
                    stream, Asrc, Bsrc, bias, out, cs, (int)M, Kgemm,
                    n_channels, stats, bn, addin);
            else
                hipLaunchKernelGGL(
                    (k_conv_gemm<MODE, 64, 4, 1, STRIDE1, CBM, false, true>),
                    dim3(grid_m, ceil_div_i(n_channels, 64)), dim3(256), 0,
                    stream, Asrc, Bsrc, bias, out, cs, (int)M, Kgemm,
                    n_channels, stats, bn, addin);
            HIP_CHECK_LAST();
            return;
        }
    }
    if (n_channels >= 128 && !narrow)
        hipLaunchKernelGGL((k_conv_gemm<MODE, 128, 2, 2, STRIDE1>),
                           dim3(grid_m, ceil_div_i(n_channels, 128)),
                           dim3(256), 0, stream, Asrc, Bsrc, bias, out, cs,
                           (int)M, Kgemm, n_channels, stats, bn, addin);
    else
        hipLaunchKernelGGL((k_conv_gemm<MODE, 64, 4, 1, STRIDE1>),
                           dim3(grid_m, ceil_div_i(n_channels, 64)),
                           dim3(256), 0, stream, Asrc, Bsrc, bias, out, cs,
                           (int)M, Kgemm, n_channels, stats, bn, addin);
    HIP_CHECK_LAST();
}

static void launch_conv_gemm_cls(hipStream_t stream, int grid_m,
                                 int n_channels, int ncls, const bf16* Asrc,
                                 const bf16* Bsrc, bf16* out,
                                 const ClsPack& pack) {
    if (n_channels >= 128)
        hipLaunchKernelGGL((k_conv_gemm_cls<128, 2, 2>),
                           dim3(grid_m, ceil_div_i(n_channels, 128), ncls),
                           dim3(256), 0, stream, Asrc, Bsrc, out, pack,
                           n_channels);
    else
        hipLaunchKernelGGL((k_conv_gemm_cls<64, 4, 1>),
                           dim3(grid_m, ceil_div_i(n_channels, 64), ncls),
                           dim3(256), 0, stream, Asrc, Bsrc, out, pack,
                           n_channels);
    HIP_CHECK_LAST();
}

// y, and with want_stats the per-channel partial sum / sumsq slab
// [2][Ko][gridM] for the consuming BN (SURVEY §7 "fuse normalisation work
// into the producing kernel"), which needs the MFMA conv.
static std::vector<at::Tensor> conv_fwd_impl(
        const at::Tensor& x, const at::Tensor& w,
        const c10::optional<at::Tensor>& bias, long stride, long pad,
        bool want_stats, long kwalk) {
    // x: NCHW logical / channels_last physical bf16; w: KCRS logical /
    // channels_last physical (= KRSC memory) bf16
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16);
    ConvShape cs = make_shape(x, w.size(0), w.size(2), w.size(3),
                              (int)stride, (int)pad);
    int Kgemm = cs.R * cs.S * cs.C;
    long M = (long)cs.N * cs.P * cs.Q;
    auto stream = at::hip::getCurrentHIPStream();
    const float* bp = bias.has_value() ? bias->data_ptr<float>() : nullptr;
    const bf16* xp = reinterpret_cast<const bf16*>(x.data_ptr());
    const bf16* wp = reinterpret_cast<const bf16*>(w.data_ptr());
    auto y = empty_nhwc(x, cs.N, cs.Ko, cs.P, cs.Q);
    bf16* yp = reinterpret_cast<bf16*>(y.data_ptr());

    if (cs.C < 8 && !want_stats) {
        plan_kloop(0, cs, kwalk);           // validates kwalk
        TORCH_CHECK(cs.Ko % 8 == 0);
        int lds = cs.Ko * Kgemm * 2;
        long total = M * (cs.Ko / 8);
        int blocks = std::min<long>(8192, ceil_div_i(total, 256));
        hipLaunchKernelGGL(k_conv_small_cin, dim3(blocks), dim3(256), lds,
                           stream.stream(), xp, wp, bp, yp, cs, M);
        HIP_CHECK_LAST();
        return {y, at::Tensor()};
    }
    TORCH_CHECK(cs.C % 8 == 0, want_stats
                ? "stats path needs the MFMA conv (C%8==0)"
                : "conv fwd needs C % 8 == 0");
    // the staged epilogue stores 16 B (8-channel) chunks per row
    TORCH_CHECK(cs.Ko % 8 == 0, "conv fwd needs Ko % 8 == 0");
    const int gridM = ceil_div_i(M, CBM);
    at::Tensor slab;
    if (want_stats)
        slab = at::empty({2, (long)cs.Ko, (long)gridM},
                         x.options().dtype(at::kFloat));
    static const char* tbn_env = getenv("DDPX_CONV_TBN64");
    launch_conv_gemm<0>(stream.stream(), gridM, cs.Ko,
                        tbn_env && !want_stats, xp, wp, bp, yp, cs, M, Kgemm,
                        want_stats ? slab.data_ptr<float>() : nullptr,
                        BnFuse{}, nullptr, kwalk);
    return {y, slab};
}

at::Tensor conv2d_fwd(at::Tensor x, at::Tensor w,
                      c10::optional<at::Tensor> bias, long stride, long pad,
                      long kwalk) {
    return conv_fwd_impl(x, w, bias, stride, pad, false, kwalk)[0];
}

std::vector<at::Tensor> conv2d_fwd_stats(at::Tensor x, at::Tensor w,
                                         c10::optional<at::Tensor> bias,
                                         long stride, long pad, long kwalk) {
    return conv_fwd_impl(x, w, bias, stride, pad, true, kwalk);
}

// dy: NCHW logical / channels_last bf16 [N,Ko,P,Q]; wt2: [C, R*S*Ko] bf16
static ConvShape dgrad_shape(const at::Tensor& dy, long N, long C, long H,
                             long W, long R, long S, long stride, long pad) {
    ConvShape cs;
    cs.N = N; cs.C = C; cs.H = H; cs.W = W;
    cs.Ko = dy.size(1); cs.P = dy.size(2); cs.Q = dy.size(3);
    cs.R = R; cs.S = S; cs.stride = stride; cs.pad = pad;
    init_fastdiv(cs);
    TORCH_CHECK(cs.Ko % 8 == 0, "conv dgrad needs Ko % 8 == 0");
    // the staged epilogue stores 16 B (8-channel) chunks per dx row
    TORCH_CHECK(cs.C % 8 == 0, "conv dgrad needs C % 8 == 0");
    return cs;
}

struct DgradPlan {
    const char* name;   // "raster" or "taps"
    int G;              // taps: images per row group; raster: 0
    long k_tiles, k_tiles_raster;   // K-tiles issued per column of M-tiles
};

// Row order of the stride-1 dgrad: every dispatch decision is made here and
// nowhere else.  Pure host arithmetic.  group: -1 automatic, 0 raster, 32 /
// 64 / 128 forces that G; a forced G on a shape the tap-uniform order does
// not fit runs raster, and the plan says so.  `raster` whenever stride != 1,
// Ko % 64 != 0 (a K-tile would straddle taps), R*S > 32 (mask bits), N % G
// != 0, a BN slab is requested (the slab epilogue indexes raster tiles), or
// the tap model skips nothing (1x1, valid == all).  The automatic choice is
// MEASURED (tools/bench_kernels.py --dgradtaps, docs/KERNELS.md): a shape
// class no measurement showed faster stays raster.
static DgradPlan plan_dgrad(const ConvShape& cs, bool want_bn, long group) {
    TORCH_CHECK(group == -1 || group == 0 || group == 32 || group == 64 ||
                group == 128, "conv dgrad group must be -1 (automatic), 0 "
                "(raster), 32, 64 or 128; got ", group);
    const long M = (long)cs.N * cs.H * cs.W;
    const int tiles = ceil_div_i(M, CBM);
    DgradPlan p{"raster", 0, 0, 0};
    p.k_tiles_raster = (long)tiles * ceil_div_i((long)cs.R * cs.S * cs.Ko, CBK);
    p.k_tiles = p.k_tiles_raster;
    const bool fits = cs.stride == 1 && cs.Ko % CBK == 0 &&
                      cs.R * cs.S <= 32 && !want_bn && M < INT_MAX;
    if (!fits || group == 0) return p;

    auto count = [&](int G) {           // K-tiles the masked loop issues
        int lg = 0;
        while ((1 << lg) < G) ++lg;
        // where tiles do not straddle image groups every group has the
        // same masks: count one and multiply (this runs on every dgrad call)
        const long ghw = (long)G * cs.H * cs.W;
        const bool periodic = ghw % CBM == 0;
        const int walk = periodic ? (int)(ghw / CBM) : tiles;
        long n = 0;
        for (int t = 0; t < walk; ++t) {
            const int m0 = t * CBM;
            const int m1 = (int)std::min<long>(m0 + CBM, M) - 1;
            n += __builtin_popcount(dgrad_tap_mask(
                m0, m1, (int)ghw, lg, cs.H, cs.W, cs.P, cs.Q, cs.R, cs.S,
                cs.pad));
        }
        if (periodic) n *= cs.N / G;
        return n * (cs.Ko / CBK);
    };
    // Automatic: only the shape classes the micro-benchmark showed faster
    // by several times its spread, at the batch it ran them (B = 1024; more
    // images only add tiles of the same kind).  Toy_Net conv3 131.7 -> 91.1
    // us, conv4 306.8 -> 230.5 at G = 128; conv2 (179.6 -> 166.9, inside
    // 1.3x the spread) and every shape not measured stay raster.
    static const struct { int C, H, W, Ko, R, S, pad, G; } MEASURED[] = {
        {128, 12, 12, 256, 3, 3, 0, 128},     // Toy_Net conv3
        {256, 10, 10, 512, 3, 3, 0, 128},     // Toy_Net conv4
    };
    int G = (int)std::max<long>(group, 0);
    if (group < 0 && cs.N >= 1024)
        for (const auto& m : MEASURED)
            if (cs.C == m.C && cs.H == m.H && cs.W == m.W && cs.Ko == m.Ko &&
                cs.R == m.R && cs.S == m.S && cs.pad == m.pad)
                G = m.G;
    if (G == 0 || cs.N % G != 0) return p;
    const long issued = count(G);
    if (issued >= p.k_tiles_raster) return p;
    p.name = "taps";
    p.G = G;
    p.k_tiles = issued;
    return p;
}

// Stride-1 dgrad.  addend: optional bf16 channels_last [N,C,H,W] streamed
// into the epilogue (dx += addend — the fused ResNet skip-grad).  bn: with
// bn.slab set the epilogue also emits the upstream BN's backward partials.
static at::Tensor dgrad_stride1(const at::Tensor& dy, const at::Tensor& wt2,
                                ConvShape cs,
                                const c10::optional<at::Tensor>& addend,
                                BnFuse bn, long group, long kwalk) {
    auto dx = empty_nhwc(dy, cs.N, cs.C, cs.H, cs.W);
    const bf16* adp = nullptr;
    if (addend.has_value()) {
        TORCH_CHECK(addend->sizes() == dx.sizes() &&
                    addend->scalar_type() == at::kBFloat16);
        adp = reinterpret_cast<const bf16*>(addend->data_ptr());
    }
    const long M = (long)cs.N * cs.H * cs.W;
    const int grid_m = ceil_div_i(M, CBM);
    const int Kgemm = cs.R * cs.S * cs.Ko;
    auto stream = at::hip::getCurrentHIPStream().stream();
    const bf16* dyp = reinterpret_cast<const bf16*>(dy.data_ptr());
    const bf16* wtp = reinterpret_cast<const bf16*>(wt2.data_ptr());
    bf16* dxp = reinterpret_cast<bf16*>(dx.data_ptr());
    const DgradPlan plan = plan_dgrad(cs, bn.slab != nullptr, group);
    if (plan.G == 0) {
        launch_conv_gemm<1>(stream, grid_m, cs.C, false, dyp, wtp, nullptr,
                            dxp, cs, M, Kgemm, nullptr, bn, adp, kwalk);
        return dx;
    }
    // tap-uniform row order: same tiles, grid and arguments, rows permuted
    cs.fdGHW.init((unsigned)plan.G * cs.H * cs.W);
    cs.lgG = 0;
    while ((1 << cs.lgG) < plan.G) ++cs.lgG;
    const bool walk = plan_kloop(1, cs, kwalk)[0] == 'w';
    const dim3 grid(grid_m, ceil_div_i(cs.C, cs.C >= 128 ? 128 : 64));
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, dyp, wtp,
                           (const float*)nullptr, dxp, cs, (int)M, Kgemm,
                           cs.C, (float*)nullptr, BnFuse{}, adp);
    };
    if (cs.C >= 128) {
        if (walk) launch(k_conv_gemm<1, 128, 2, 2, true, CBM, true, true>);
        else launch(k_conv_gemm<1, 128, 2, 2, true, CBM, true, false>);
    } else {
        if (walk) launch(k_conv_gemm<1, 64, 4, 1, true, CBM, true, true>);
        else launch(k_conv_gemm<1, 64, 4, 1, true, CBM, true, false>);
    }
    HIP_CHECK_LAST();
    return dx;
}

at::Tensor conv2d_dgrad(at::Tensor dy, at::Tensor wt2, long N, long C,
                        long H, long W, long R, long S, long stride, long pad,
                        c10::optional<at::Tensor> addend, long group,
                        long kwalk) {
    ConvShape cs = dgrad_shape(dy, N, C, H, W, R, S, stride, pad);
    TORCH_CHECK(!addend.has_value() || cs.stride == 1,
                "fused dgrad addend needs stride 1");
    if (cs.stride == 1)
        return dgrad_stride1(dy, wt2, cs, addend, BnFuse{}, group, kwalk);
    plan_dgrad(cs, false, group);       // validates group; strided is raster
    plan_kloop(1, cs, kwalk);           // validates kwalk; strided is decode

    // NOTE: zero-stuffing dy to reach the stride-1 gather was tried and
    // REVERTED — measured slower at ResNet's strided shapes (r18 3x3/2:
    // 113 vs 99 us, 1x1/2: 44 vs 22 us): the 4x stuffed-dy traffic costs
    // more than the divisibility-checked gather saves.
    auto dx = empty_nhwc(dy, cs.N, cs.C, cs.H, cs.W);
    auto stream = at::hip::getCurrentHIPStream();
    const bf16* dyp_ = reinterpret_cast<const bf16*>(dy.data_ptr());
    const bf16* wt2p = reinterpret_cast<const bf16*>(wt2.data_ptr());
    bf16* dxp = reinterpret_cast<bf16*>(dx.data_ptr());
    // stride > 1: sub-grid class decomposition — one MODE-2 launch per
    // (a, b) residue class, each summing ONLY its contributing taps
    // (the divisibility-checked single launch wastes stride^2 x MFMA work
    // on zero taps: measured 97 vs ~400 TFLOP/s against stride-1 shapes)
    const int st = cs.stride;
    // classes with no contributing taps leave their dx sub-grid untouched
    // (e.g. 1x1/2: only class (0,0) exists) — pre-zero dx if any are empty
    {
        bool any_empty = false;
        for (int a = 0; a < st && !any_empty; ++a) {
            int nr = 0;
            for (int r = 0; r < cs.R; ++r)
                if (((a + cs.pad - r) % st + st) % st == 0) ++nr;
            if (nr == 0) any_empty = true;
        }
        if (!any_empty)
            for (int b = 0; b < st && !any_empty; ++b) {
                int ns = 0;
                for (int sidx = 0; sidx < cs.S; ++sidx)
                    if (((b + cs.pad - sidx) % st + st) % st == 0) ++ns;
                if (ns == 0) any_empty = true;
            }
        if (any_empty) dx.zero_();
    }
    // Build the per-class shapes; classes merge into ONE launch with
    // blockIdx.z = class when they fit the 4-slot pack (stride 2 — every
    // ResNet site); larger strides launch per class.
    ClsPack pack{};
    int ncls = 0;
    int maxTiles = 0;
    for (int a = 0; a < st; ++a) {
        for (int b = 0; b < st; ++b) {
            ConvShape c2 = cs;
            c2.cls_a = a; c2.cls_b = b;
            c2.Hfull = cs.H; c2.Wfull = cs.W;
            c2.nr = 0; c2.ns = 0;
            for (int r = 0; r < cs.R; ++r)
                if (((a + cs.pad - r) % st + st) % st == 0) {
                    c2.taps_r[c2.nr] = r;
                    // exact division by construction (C division truncates
                    // toward zero, but the value is an exact multiple)
                    c2.off_r[c2.nr] = (a + cs.pad - r) / st;
                    ++c2.nr;
                }
            for (int sidx = 0; sidx < cs.S; ++sidx)
                if (((b + cs.pad - sidx) % st + st) % st == 0) {
                    c2.taps_s[c2.ns] = sidx;
                    c2.off_s[c2.ns] = (b + cs.pad - sidx) / st;
                    ++c2.ns;
                }
            if (c2.nr == 0 || c2.ns == 0) continue;  // dx pre-zeroed above
            int Ha = (cs.H - a + st - 1) / st;
            int Wb = (cs.W - b + st - 1) / st;
            c2.H = Ha; c2.W = Wb;           // fdH/fdW decode the class grid
            c2.fdH.init(Ha); c2.fdW.init(Wb);
            c2.fdNs.init(c2.ns);
            long M2 = (long)cs.N * Ha * Wb;
            int K2 = c2.nr * c2.ns * cs.Ko;
            if (ncls < 4) {
                pack.cs[ncls] = c2;
                pack.M[ncls] = (int)M2;
                pack.K[ncls] = K2;
                maxTiles = std::max(maxTiles, (int)ceil_div_i(M2, CBM));
                ++ncls;
            } else {
                // >4 contributing classes (stride > 2): per-class launch
                launch_conv_gemm<2>(stream.stream(), ceil_div_i(M2, CBM),
                                    cs.C, false, dyp_, wt2p, nullptr, dxp,
                                    c2, M2, K2, nullptr, BnFuse{}, nullptr);
            }
        }
    }
    if (ncls > 0)
        launch_conv_gemm_cls(stream.stream(), maxTiles, cs.C, ncls, dyp_,
                             wt2p, dxp, pack);
    return dx;
}

std::vector<at::Tensor> conv2d_dgrad_bn(at::Tensor dy, at::Tensor wt2,
                                        long N, long C, long H, long W,
                                        long R, long S, long pad,
                                        at::Tensor bn_x, at::Tensor bn_mask,
                                        at::Tensor bn_mean,
                                        at::Tensor bn_invstd) {
    // stride-1 dgrad that ALSO emits the upstream BN's backward partial
    // sums ([2][C][gridM], fed to bn_bwd's pre_slab) — the BN partial pass
    // never re-reads x/dy.
    ConvShape cs = dgrad_shape(dy, N, C, H, W, R, S, 1, pad);
    const int gridM = ceil_div_i((long)cs.N * cs.H * cs.W, CBM);
    auto slab = at::empty({2, (long)cs.C, (long)gridM},
                          dy.options().dtype(at::kFloat));
    BnFuse bn;
    bn.x = reinterpret_cast<const bf16*>(bn_x.data_ptr());
    bn.mask = bn_mask.numel()
        ? bn_mask.data_ptr<unsigned char>() : nullptr;
    bn.mean = bn_mean.data_ptr<float>();
    bn.invstd = bn_invstd.data_ptr<float>();
    bn.slab = slab.data_ptr<float>();
    return {dgrad_stride1(dy, wt2, cs, c10::nullopt, bn, -1, -1), slab};
}

// (name, G, k_tiles_issued, k_tiles_raster) conv2d_dgrad would run for this
// shape and group argument; no tensors, launches nothing.  The counts are
// K-tiles summed over the M-tiles of one tile column: issued is popcount of
// each tile's tap mask times Ko/64 (the raster count when the plan is
// raster), so a mask wider than the tile's pixels need shows up here.
std::tuple<std::string, long, long, long> conv2d_dgrad_plan(
        long N, long C, long H, long W, long Ko, long R, long S, long stride,
        long pad, long group) {
    TORCH_CHECK(N > 0 && C > 0 && Ko > 0 && R > 0 && S > 0 && stride > 0 &&
                pad >= 0 && H + 2 * pad >= R && W + 2 * pad >= S);
    ConvShape cs = make_shape((int)N, (int)C, (int)H, (int)W, (int)Ko, (int)R,
                              (int)S, (int)stride, (int)pad);
    const DgradPlan p = plan_dgrad(cs, false, group);
    return std::make_tuple(std::string(p.name), (long)p.G, p.k_tiles,
                           p.k_tiles_raster);
}

// "walk" or "decode": the K loop conv2d_fwd[_stats] (mode 0) or conv2d_dgrad
// (mode 1) would run for this shape and kwalk argument; no tensors, launches
// nothing.
std::string conv2d_kloop_plan(long mode, long N, long C, long H, long W,
                              long Ko, long R, long S, long stride, long pad,
                              long kwalk) {
    TORCH_CHECK(mode == 0 || mode == 1, "mode is 0 (forward) or 1 (dgrad)");
    TORCH_CHECK(N > 0 && C > 0 && Ko > 0 && R > 0 && S > 0 && stride > 0 &&
                pad >= 0 && H + 2 * pad >= R && W + 2 * pad >= S);
    ConvShape cs = make_shape((int)N, (int)C, (int)H, (int)W, (int)Ko, (int)R,
                              (int)S, (int)stride, (int)pad);
    return plan_kloop((int)mode, cs, kwalk);
}

at::Tensor col_sum(at::Tensor x);   // gemm.hip

// ----------------------------------------------------------- wgrad hosts ---

enum class WgradLeaf {
    StemStream, C1R3, SmallRsc, SmallCin,       // C < 8: VALU kernels
    SbPair32, SbPair64,                         // MFMA, 64x64 tile
    WidePair32, WidePair64, WideDma32, WideDma64,   // MFMA, 128x128 tile
};

// indexed by WgradLeaf: name, and for the MFMA leaves (one signature, one
// grid) the kernel without / with the fused bias partials
using WgradMfmaKernel = void (*)(const bf16*, const bf16*, float*, ConvShape,
                                 long, int, int);
static const struct { const char* name; WgradMfmaKernel kern[2]; }
WGRAD_LEAVES[] = {
    {"c1_r3_stream", {}}, {"c1_r3", {}}, {"small_rsc", {}}, {"small_cin", {}},
    {"sb_pair<32>", {k_conv_wgrad_sb_pair<32>, k_conv_wgrad_sb_pair<32>}},
    {"sb_pair<64>", {k_conv_wgrad_sb_pair<64>, k_conv_wgrad_sb_pair<64>}},
    {"wide_pair<32>", {k_conv_wgrad_wide_pair<32, false>,
                       k_conv_wgrad_wide_pair<32, true>}},
    {"wide_pair<64>", {k_conv_wgrad_wide_pair<64, false>,
                       k_conv_wgrad_wide_pair<64, true>}},
    {"wide_dma<32>", {k_conv_wgrad_wide_dma<32, false>,
                      k_conv_wgrad_wide_dma<32, true>}},
    {"wide_dma<64>", {k_conv_wgrad_wide_dma<64, false>,
                      k_conv_wgrad_wide_dma<64, true>}},
};
static_assert(sizeof(WGRAD_LEAVES) / sizeof(WGRAD_LEAVES[0]) ==
              (int)WgradLeaf::WideDma64 + 1, "one row per WgradLeaf");

struct WgradPlan {
    WgradLeaf leaf;
    int S;              // split count = slab slices the combine sums
    int gk, gr;         // MFMA leaves: ko / rsc tile counts, grid (gk, gr, S)
    bool fused_bias;    // db comes out of the wgrad and combine launches;
                        // otherwise it is a separate column sum over dy
};

// DDPX_WGRAD_V, read once per process
static const char* wgrad_override() {
    static const char* v = getenv("DDPX_WGRAD_V");
    return v;
}

// Which kernel runs for this shape, and how deep it splits: every wgrad
// dispatch decision is made here and nowhere else.  Pure host arithmetic —
// no device, no allocation.  The choice is MEASURED (profiles/,
// tools/bench_kernels.py):
//   * C < 8 takes a VALU kernel whatever the override says;
//   * 128x128 wide tile, LDS-DMA staged (wide_dma), 64-deep, for big-Kgemm
//     convs with enough tiles (with bias: conv3 119 vs 174 us pair-store,
//     conv4 235 vs 384);
//   * the same tile 32-DEEP for small-Kgemm or tile-starved-but-deep-M
//     shapes (conv2 218 vs 282 us pair-store);
//   * 64x64 pair-store sb_pair otherwise.
// override (DDPX_WGRAD_V) forces an MFMA leaf for A/B runs: wt = wide_dma at
// the automatic depth, wt3 = wide_dma<32>, wp = wide_pair<64>, wq =
// wide_pair<32> (the pair-store leaves wide_dma replaced, profiles/
// toynet_b1024_1gpu_kernel_stats_wgraddma.md), s / sb = sb_pair<32>, s6 =
// sb_pair<64>.  A wide leaf forced on a shape the 128x128 tile does not fit
// runs sb_pair<32>.  Any other value is an error.
static WgradPlan plan_wgrad(const ConvShape& cs, long M, bool want_bias,
                            const char* override) {
    enum { Auto, Dma, Dma32, Pair64, Pair32, Sb32, Sb64 } force = Auto;
    if (override && override[0]) {
        const std::string v(override);
        if (v == "wt") force = Dma;
        else if (v == "wt3") force = Dma32;
        else if (v == "wp") force = Pair64;
        else if (v == "wq") force = Pair32;
        else if (v == "s" || v == "sb") force = Sb32;
        else if (v == "s6") force = Sb64;
        else TORCH_CHECK(false, "DDPX_WGRAD_V=", v, " selects no wgrad "
                         "kernel; accepted values: wt, wt3, wp, wq, s, sb, "
                         "s6 (unset or empty: automatic)");
    }
    const int Kgemm = cs.R * cs.S * cs.C;
    WgradPlan p{};

    if (cs.C < 8) {
        const bool c1r3 = cs.C == 1 && cs.R == 3 && cs.S == 3;
        if (c1r3 && cs.Ko % 8 == 0 && cs.Ko <= 64 && M < INT_MAX) {
            // work is dealt in wave loads (rpl rows); a block wants >= 2
            // trips per wave, and 768 blocks = 3 per CU (the occupancy the
            // kernel's registers allow) all stream at once
            const int rpl = 64 / (cs.Ko / 8);
            const long nloads = (M + rpl - 1) / rpl;
            p.leaf = WgradLeaf::StemStream;
            p.S = (int)std::max<long>(
                1, std::min<long>(768, (nloads + 8 * SU - 1) / (8 * SU)));
            p.fused_bias = want_bias;
        } else if (Kgemm <= 16 && cs.Ko <= 64) {
            // S=8192 measured slower (164 vs 132 us): per-block reduction
            // fixed costs dominate below ~80 rows/walker
            p.leaf = c1r3 ? WgradLeaf::C1R3 : WgradLeaf::SmallRsc;
            p.S = (int)std::max<long>(1, std::min<long>(2048, M / 8));
        } else {
            p.leaf = WgradLeaf::SmallCin;
            p.S = 64;
        }
        return p;
    }

    TORCH_CHECK(cs.C % 8 == 0 && cs.Ko % 8 == 0);
    const bool can_wide = cs.Ko >= 128 && Kgemm >= 128;
    const bool enough = can_wide &&
        (ceil_div_i(cs.Ko, 128) * ceil_div_i(Kgemm, 128) >= 8
         || M >= 262144);
    const bool wide = force == Auto
        ? enough
        : can_wide && force != Sb32 && force != Sb64;
    const int tile = wide ? 128 : WBM;
    p.gk = ceil_div_i(cs.Ko, tile);
    p.gr = ceil_div_i(Kgemm, tile);
    if (wide) {
        const bool deep = Kgemm >= 1152;
        p.leaf = force == Pair64 ? WgradLeaf::WidePair64
               : force == Pair32 ? WgradLeaf::WidePair32
               : force == Dma32 || !deep ? WgradLeaf::WideDma32
               : WgradLeaf::WideDma64;
    } else {
        // single-ko-tile shapes: 64-deep staging measured faster (1x1
        // [64x64,M=800k] 166 vs 174 us; 7x7 stem 209 vs 215)
        const bool sb64 = force == Auto ? p.gk == 1 && p.gr <= 8
                                        : force == Sb64;
        p.leaf = sb64 ? WgradLeaf::SbPair64 : WgradLeaf::SbPair32;
    }
    // The loop counts contraction steps 64 deep for EVERY wide leaf and 32
    // deep for EVERY sb leaf, whatever the leaf's own DEPTH (wide_dma<32>,
    // wide_pair<32> and sb_pair<64> included).  Odd, but S fixes the
    // summation order and so the bits of dw; the exact tests pin it.
    const int count_depth = wide ? 64 : 32;
    p.S = 1;
    // split until the machine fills (256 CUs x several blocks); small tile
    // grids (1x1 convs: one 64x64 tile) need deep splits — measured 17
    // TFLOP/s at the old S<=64 cap on [Ko=64,C=64] wgrad
    // deepen splits until ~1024 blocks, but keep >=8 contraction steps per
    // block (measured: S=512 at M=65k quadrupled a 55 us wgrad)
    // (cap 2048 measured worse: the S-sweep in the combine pass dominates
    // — 281 vs 174 us at [Ko=64,C=64,M=800k])
    while (p.gk * p.gr * p.S < 1024 && p.S < 512 &&
           M / ((long)p.S * 2 * count_depth) >= 8) p.S *= 2;
    // the wide leaves emit S x Ko bias partials behind the dw slices
    p.fused_bias = want_bias && wide;
    return p;
}

// (leaf name, split, fused_bias) that conv2d_wgrad / conv2d_wgrad_bias would
// run for this shape under this process's DDPX_WGRAD_V; launches nothing
std::tuple<std::string, long, bool> conv2d_wgrad_plan(
        long N, long C, long H, long W, long Ko, long R, long S, long stride,
        long pad, bool want_bias) {
    TORCH_CHECK(N > 0 && C > 0 && Ko > 0 && R > 0 && S > 0 && stride > 0 &&
                pad >= 0 && H + 2 * pad >= R && W + 2 * pad >= S);
    ConvShape cs = make_shape((int)N, (int)C, (int)H, (int)W, (int)Ko, (int)R,
                              (int)S, (int)stride, (int)pad);
    WgradPlan p = plan_wgrad(cs, (long)cs.N * cs.P * cs.Q, want_bias,
                             wgrad_override());
    return std::make_tuple(std::string(WGRAD_LEAVES[(int)p.leaf].name),
                           (long)p.S, p.fused_bias);
}

// dw, and with want_bias also db = sum of dy over (n, p, q): plan, allocate,
// launch, combine.  The leaves Toy_Net runs (wide_dma<32>, wide_dma<64>, the
// streaming stem kernel) produce db inside the wgrad and combine launches;
// every other leaf takes the separate column-sum pass over dy.
static std::vector<at::Tensor> wgrad_impl(const at::Tensor& dy,
                                          const at::Tensor& x, long R,
                                          long S, long stride, long pad,
                                          bool want_bias) {
    ConvShape cs = make_shape(x, dy.size(1), (int)R, (int)S, (int)stride,
                              (int)pad);
    TORCH_CHECK(cs.P == dy.size(2) && cs.Q == dy.size(3));
    const long M = (long)cs.N * cs.P * cs.Q;
    const int Kgemm = cs.R * cs.S * cs.C;
    const WgradPlan plan = plan_wgrad(cs, M, want_bias, wgrad_override());
    const int S_ = plan.S;
    const bool fused_bias = plan.fused_bias;

    auto stream = at::hip::getCurrentHIPStream();
    const auto f32 = x.options().dtype(at::kFloat);
    auto dw = at::empty({(long)cs.Ko, (long)cs.C, (long)cs.R, (long)cs.S},
                        f32);
    at::Tensor db;
    if (fused_bias) db = at::empty({(long)cs.Ko}, f32);
    float* dbp = fused_bias ? db.data_ptr<float>() : nullptr;
    const bf16* dyp = reinterpret_cast<const bf16*>(dy.data_ptr());
    const bf16* xp = reinterpret_cast<const bf16*>(x.data_ptr());

    switch (plan.leaf) {
    case WgradLeaf::StemStream:
    case WgradLeaf::C1R3:
    case WgradLeaf::SmallRsc: {
        // slab [taps][Ko][S_], one combine for all three; the stem kernel
        // with bias carries db as one more "tap"
        const int nt = Kgemm + fused_bias;
        auto slab = at::empty({nt * cs.Ko, S_}, f32);
        if (plan.leaf == WgradLeaf::StemStream) {
            const int rpl = 64 / (cs.Ko / 8);
            const long nloads = (M + rpl - 1) / rpl;
            const long chunk = (nloads + 4L * S_ - 1) / (4L * S_) * rpl;
            auto kern = want_bias
                ? (cs.pad ? k_wgrad_c1_r3_stream<true, true>
                          : k_wgrad_c1_r3_stream<true, false>)
                : (cs.pad ? k_wgrad_c1_r3_stream<false, true>
                          : k_wgrad_c1_r3_stream<false, false>);
            hipLaunchKernelGGL(kern, dim3(S_), dim3(256), 0, stream.stream(),
                               dyp, xp, slab.data_ptr<float>(), cs, M, chunk);
        } else if (plan.leaf == WgradLeaf::C1R3) {
            hipLaunchKernelGGL(k_wgrad_c1_r3, dim3(S_), dim3(256), 0,
                               stream.stream(), dyp, xp,
                               slab.data_ptr<float>(), cs, M, S_);
        } else {
            hipLaunchKernelGGL(k_wgrad_small_rsc, dim3(S_), dim3(256), 0,
                               stream.stream(), dyp, xp,
                               slab.data_ptr<float>(), cs, M, S_, Kgemm);
        }
        HIP_CHECK_LAST();
        hipLaunchKernelGGL(k_wgrad_small_rsc_combine,
                           dim3(ceil_div_i(nt * cs.Ko, 4)), dim3(256), 0,
                           stream.stream(), slab.data_ptr<float>(), S_, cs,
                           Kgemm, dw.data_ptr<float>(), dbp);
        HIP_CHECK_LAST();
        break;
    }
    case WgradLeaf::SmallCin: {
        auto slab = at::empty({S_, Kgemm, cs.Ko}, f32);
        hipLaunchKernelGGL(k_wgrad_small_cin,
                           dim3(Kgemm, S_, ceil_div_i(cs.Ko, 64)), dim3(256),
                           0, stream.stream(), dyp, xp,
                           slab.data_ptr<float>(), cs, M, S_);
        HIP_CHECK_LAST();
        hipLaunchKernelGGL(k_wgrad_small_combine,
                           dim3(ceil_div_i(Kgemm * cs.Ko, 256)), dim3(256), 0,
                           stream.stream(), slab.data_ptr<float>(), S_, cs,
                           Kgemm, dw.data_ptr<float>());
        HIP_CHECK_LAST();
        break;
    }
    default: {
        // MFMA leaves: S_ slices of [Ko][Kgemm], then (fused bias) S_ x Ko
        // bias partials; past 16 slices the combine runs in two stages
        const long total = (long)cs.Ko * Kgemm;
        const long bias_ld = fused_bias ? cs.Ko : 0;
        auto slab = at::empty({S_ * (total + bias_ld)}, f32);
        hipLaunchKernelGGL(WGRAD_LEAVES[(int)plan.leaf].kern[fused_bias],
                           dim3(plan.gk, plan.gr, S_), dim3(256), 0,
                           stream.stream(), dyp, xp, slab.data_ptr<float>(),
                           cs, M, Kgemm, S_);
        HIP_CHECK_LAST();
        at::Tensor slab_f = slab;
        int S_c = S_;
        if (S_ > 16) {
            constexpr int CH = 8;
            const int chunks = ceil_div_i(S_, CH);
            auto slab2 = at::empty({chunks * (total + bias_ld)}, f32);
            const int blocks1 = (int)((total + bias_ld + 255) / 256);
            auto stage = fused_bias ? k_wgrad_combine_stage<true>
                                    : k_wgrad_combine_stage<false>;
            hipLaunchKernelGGL(stage, dim3(blocks1, chunks), dim3(256), 0,
                               stream.stream(), slab.data_ptr<float>(), S_,
                               CH, total, cs.Ko, slab2.data_ptr<float>());
            HIP_CHECK_LAST();
            slab_f = slab2;
            S_c = chunks;
        }
        // fused bias: one block more, which sums the bias partials
        const int blocks = std::min<long>(4096, ceil_div_i(total, 256));
        auto combine = fused_bias ? k_wgrad_combine<true>
                                  : k_wgrad_combine<false>;
        hipLaunchKernelGGL(combine, dim3(blocks + fused_bias), dim3(256), 0,
                           stream.stream(), slab_f.data_ptr<float>(), S_c,
                           cs, Kgemm, dw.data_ptr<float>(), dbp);
        HIP_CHECK_LAST();
    }
    }
    if (want_bias && !fused_bias)
        db = col_sum(dy.permute({0, 2, 3, 1}).reshape({M, (long)cs.Ko}));
    return {dw, db};
}

at::Tensor conv2d_wgrad(at::Tensor dy, at::Tensor x, long R, long S,
                        long stride, long pad) {
    return wgrad_impl(dy, x, R, S, stride, pad, false)[0];
}

// dw as conv2d_wgrad (bit-identical on the MFMA leaves), plus the bias
// gradient db[ko] = sum over (n, p, q) of dy, fp32
std::vector<at::Tensor> conv2d_wgrad_bias(at::Tensor dy, at::Tensor x,
                                          long R, long S, long stride,
                                          long pad) {
    return wgrad_impl(dy, x, R, S, stride, pad, true);
}
