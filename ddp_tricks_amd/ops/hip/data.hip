// data.hip — device-resident dataset: fused gather / crop / flip / normalise.
//
// One launch builds a training batch from a uint8 HWC store that lives on
// the device: gather by dataset index, random crop out of a P-pixel padded
// canvas, horizontal flip, per-channel normalisation through a 256-entry
// table, bf16 channels_last output (exactly the stem conv's operand), and
// the label gather.  Replaces, per step, the host index_select into pinned
// memory, the fp32 H2D copy and the to(bf16) + channels_last passes.
//
// The kernel does no arithmetic on pixel values: out = lut[c][u8].  The
// per-sample parameters come from a counter hash (splitmix64 finaliser)
// keyed by (seed, epoch, DATASET index), so a sample's augmentation does
// not depend on its position in the batch, the batch size or the rank:
//
//   key  = (epoch << 32) | index
//   z    = seed + (key + 1) * 0x9E3779B97F4A7C15
//   z    = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
//   z    = (z ^ (z >> 27)) * 0x94D049BB133111EB
//   z    =  z ^ (z >> 31)
//   dx   = ((z         & 0xFFFF) * (2P+1)) >> 16
//   dy   = (((z >> 16) & 0xFFFF) * (2P+1)) >> 16
//   flip = hflip ? (z >> 32) & 1 : 0
//
// torchvision order (pad, crop, flip): with xs = flip ? W-1-x : x, output
// pixel (y, x) reads source (y + dy - P, xs + dx - P); outside the image
// the value is lut[c][0] (zero padding of the raw image, then normalise).
//
// Work decomposition: a sample's output is E = H*W*C contiguous bf16.  It is
// cut into chunks of VEC elements (VEC = 8 -> one 16-byte store, aligned
// because E % 8 == 0 on that path; VEC = 1 for samples whose size is no
// multiple of 8).  64 chunks form a wave-tile; a wave owns one wave-tile at
// a time and grid-strides over all B * tiles_per_sample of them, so a wave
// never straddles two samples and (index, dx, dy, flip) are wave-uniform:
// the hash runs once per wave-tile on the scalar unit.  Each chunk decodes
// its first element's (y, x, c) with two multiply-shift divisions and steps
// the rest incrementally — fully unrolled, constant vector indices, no
// register arrays.  The LUT (C*512 bytes) is staged in LDS once per block.
//
// Indices are CLAMPED to [0, N-1] in the kernel: checking them on the host
// would need a device sync per batch.
//
// CutMix (k_batch_gather_cutmix, a sibling kernel: the launch above is
// unchanged when CutMix is off).  Still no arithmetic on pixel values: an
// output sample with dataset index i is where(box, aug(j), aug(i)), j a
// partner drawn from the WHOLE store.  Partner, apply bit and box come from
// two more counter hashes with the same (seed, epoch, index) keying and
// finaliser as above, the seed offset by a constant (arithmetic mod 2^64):
//
//   z2 = hash(seed + 0xD1B54A32D192ED03, key)      z3 = hash(seed +
//                                                  0x8CB92BA72F3D8DD7, key)
//   j     = ((z2 & 0xFFFFFFFF) * N) >> 32          uniform over [0, N)
//   r     = isqrt(z2 >> 32)                        exact floor sqrt, < 65536
//   cx    = ((z3         & 0xFFFF) * W) >> 16
//   cy    = (((z3 >> 16) & 0xFFFF) * H) >> 16
//   apply = ((z3 >> 32) & 0xFFFF) < thresh         thresh = prob in 1/65536
//   bw = (r * W) >> 16,  bh = (r * H) >> 16
//   box = [cx - bw/2, cx - bw/2 + bw) x [cy - bh/2, cy - bh/2 + bh),
//         clipped to the image; area = clipped width * clipped height
//
// r/65536 = sqrt(uniform) is the paper's alpha = 1 box (lam uniform, side
// ratio sqrt(1 - lam)), in integers only.  isqrt is a float estimate
// corrected with 64-bit integer products.  Inside the box output pixel
// (y, x) is pixel (y, x) of sample j augmented with j's OWN (dx, dy, flip)
// of that epoch; only the chosen source is read.  j, the box and both
// parameter sets are wave-uniform; box membership is decided per element,
// so a 16-byte chunk that straddles a box edge (C = 3: chunks span pixels)
// is right element by element.  Extra outputs: labels_b = labels[j]
// (labels[i] when not applied) and lam = fl32((HW - area) / HW), a
// correctly rounded fp32 division, 1.0 when not applied or the box is empty.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

#include <vector>

constexpr int DATA_BLOCK = 256;                 // 4 waves
constexpr int DATA_WAVES = DATA_BLOCK / WAVE;
constexpr int DATA_MAX_BLOCKS = 2048;
constexpr int DATA_MAX_C = 64;                  // LUT <= 32 KiB of LDS

struct AugParams {
    int dx, dy, flip;
};

DEV_INLINE AugParams aug_decode(unsigned long long seed,
                                unsigned long long epoch,
                                unsigned long long index, int pad, int hflip) {
    unsigned long long key = (epoch << 32) | index;
    unsigned long long z = seed + (key + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    const unsigned span = 2u * (unsigned)pad + 1u;
    AugParams p;
    p.dx = (int)((((unsigned)z & 0xFFFFu) * span) >> 16);
    p.dy = (int)(((((unsigned)(z >> 16)) & 0xFFFFu) * span) >> 16);
    p.flip = hflip ? (int)((z >> 32) & 1ull) : 0;
    return p;
}

template <int VEC>
__global__ __launch_bounds__(DATA_BLOCK)
void k_batch_gather_aug(const unsigned char* __restrict__ store,
                        const long* __restrict__ labels,
                        const long* __restrict__ index,
                        const unsigned short* __restrict__ lut,
                        unsigned short* __restrict__ out,
                        long* __restrict__ out_labels,
                        long N, long B, int H, int W, int C,
                        FastDiv divC, FastDiv divW,
                        unsigned chunks,          // per sample: E / VEC
                        unsigned tiles,           // per sample: wave-tiles
                        int pad, int hflip,
                        unsigned long long seed, unsigned long long epoch) {
    extern __shared__ unsigned short s_lut[];
    for (int i = threadIdx.x; i < C * 256; i += DATA_BLOCK) s_lut[i] = lut[i];
    __syncthreads();

    const int lane = threadIdx.x & (WAVE - 1);
    const long wave0 = (long)blockIdx.x * DATA_WAVES +
        __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long nwaves = (long)gridDim.x * DATA_WAVES;
    const long total = B * (long)tiles;
    const long E = (long)H * W * C;

    for (long t = wave0; t < total; t += nwaves) {
        const long b = t / tiles;                       // wave-uniform
        const unsigned tile = (unsigned)(t - b * tiles);
        long idx = index[b];
        idx = idx < 0 ? 0 : (idx >= N ? N - 1 : idx);   // documented clamp
        const AugParams ap = aug_decode(seed, epoch, (unsigned long long)idx,
                                        pad, hflip);
        if (tile == 0 && lane == 0) out_labels[b] = labels[idx];

        const unsigned k = tile * WAVE + lane;
        if (k >= chunks) continue;
        const unsigned e0 = k * VEC;
        const unsigned p0 = fd_div(e0, divC);
        int c = (int)fd_mod(e0, divC, p0);
        const unsigned y0 = fd_div(p0, divW);
        int x = (int)fd_mod(p0, divW, y0);
        int y = (int)y0;
        const unsigned char* src = store + idx * E;
        const int ox = ap.dx - pad, oy = ap.dy - pad;

        unsigned short v[VEC];
        #pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int sy = y + oy;
            const int sx = (ap.flip ? W - 1 - x : x) + ox;
            const bool in = (unsigned)sy < (unsigned)H &&
                            (unsigned)sx < (unsigned)W;
            unsigned u = 0;
            if (in) u = src[(sy * W + sx) * C + c];   // < E < 2^31
            v[j] = s_lut[c * 256 + u];
            if (++c == C) {
                c = 0;
                if (++x == W) { x = 0; ++y; }
            }
        }
        unsigned short* dst = out + b * E + e0;
        if constexpr (VEC == 8) {
            s16x8 o;
            #pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (short)v[j];
            *reinterpret_cast<s16x8*>(dst) = o;
        } else {
            dst[0] = v[0];
        }
    }
}

std::vector<at::Tensor> batch_gather_aug(at::Tensor store, at::Tensor labels,
                                         at::Tensor index, at::Tensor lut,
                                         long pad, bool hflip, long seed,
                                         long epoch) {
    TORCH_CHECK(store.is_cuda() && store.scalar_type() == at::kByte &&
                store.dim() == 4 && store.is_contiguous(),
                "store must be a contiguous uint8 [N,H,W,C] device tensor");
    const long N = store.size(0);
    const long H = store.size(1), W = store.size(2), C = store.size(3);
    TORCH_CHECK(N >= 1 && N < (1ll << 32), "store needs 1 <= N < 2^32");
    TORCH_CHECK(H >= 1 && W >= 1 && C >= 1 && C <= DATA_MAX_C,
                "store needs H, W >= 1 and 1 <= C <= ", DATA_MAX_C);
    const long E = H * W * C;
    TORCH_CHECK(E < (1ll << 31), "sample too large");
    TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong &&
                labels.dim() == 1 && labels.size(0) == N &&
                labels.is_contiguous(), "labels must be int64 [N]");
    TORCH_CHECK(index.is_cuda() && index.scalar_type() == at::kLong &&
                index.dim() == 1 && index.is_contiguous(),
                "index must be a contiguous int64 [B] device tensor");
    TORCH_CHECK(lut.is_cuda() && lut.scalar_type() == at::kBFloat16 &&
                lut.dim() == 2 && lut.size(0) == C && lut.size(1) == 256 &&
                lut.is_contiguous(), "lut must be bf16 [C,256]");
    TORCH_CHECK(labels.device() == store.device() &&
                index.device() == store.device() &&
                lut.device() == store.device(),
                "all operands must live on one device");
    TORCH_CHECK(pad >= 0 && pad <= 4096, "pad must be in [0, 4096]");
    TORCH_CHECK(epoch >= 0 && epoch < (1ll << 32), "epoch must be in [0, 2^32)");

    const long B = index.size(0);
    auto images = at::empty(
        {B, C, H, W},
        store.options().dtype(at::kBFloat16)
            .memory_format(at::MemoryFormat::ChannelsLast));
    auto out_labels = at::empty({B}, labels.options());
    if (B == 0) return {images, out_labels};

    const bool vec = (E % 8) == 0;
    const unsigned chunks = (unsigned)(vec ? E / 8 : E);
    const unsigned tiles = (chunks + WAVE - 1) / WAVE;
    const long total = B * (long)tiles;
    const int blocks = (int)std::min<long>(
        DATA_MAX_BLOCKS, (total + DATA_WAVES - 1) / DATA_WAVES);
    FastDiv divC, divW;
    divC.init((unsigned)C);
    divW.init((unsigned)W);
    const size_t lds = (size_t)C * 256 * sizeof(unsigned short);
    auto stream = at::hip::getCurrentHIPStream();
    auto kern = vec ? k_batch_gather_aug<8> : k_batch_gather_aug<1>;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(DATA_BLOCK), lds,
                       stream.stream(), store.data_ptr<unsigned char>(),
                       labels.data_ptr<long>(), index.data_ptr<long>(),
                       reinterpret_cast<const unsigned short*>(lut.data_ptr()),
                       reinterpret_cast<unsigned short*>(images.data_ptr()),
                       out_labels.data_ptr<long>(), N, B, (int)H, (int)W,
                       (int)C, divC, divW, chunks, tiles, (int)pad,
                       (int)hflip, (unsigned long long)seed,
                       (unsigned long long)epoch);
    HIP_CHECK_LAST();
    return {images, out_labels};
}

// ------------------------------------------------------------------ CutMix ---

constexpr unsigned long long MIX_SEED_A = 0xD1B54A32D192ED03ull;
constexpr unsigned long long MIX_SEED_B = 0x8CB92BA72F3D8DD7ull;

struct MixParams {
    long j;                   // partner dataset index
    int apply;
    int x0, y0, x1, y1;       // clipped box, half-open
    int area;
};

DEV_INLINE unsigned long long mix_hash(unsigned long long seed,
                                       unsigned long long epoch,
                                       unsigned long long index) {
    unsigned long long key = (epoch << 32) | index;
    unsigned long long z = seed + (key + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// exact floor(sqrt(v)) for a 32-bit v: float estimate, integer correction
DEV_INLINE unsigned isqrt32(unsigned v) {
    unsigned long long r = (unsigned long long)sqrtf((float)v);
    if (r > 65535ull) r = 65535ull;
    while (r * r > (unsigned long long)v) --r;
    while ((r + 1ull) * (r + 1ull) <= (unsigned long long)v) ++r;
    return (unsigned)r;
}

DEV_INLINE MixParams mix_decode(unsigned long long seed,
                                unsigned long long epoch,
                                unsigned long long index, long N, int H, int W,
                                unsigned thresh) {
    const unsigned long long z2 = mix_hash(seed + MIX_SEED_A, epoch, index);
    const unsigned long long z3 = mix_hash(seed + MIX_SEED_B, epoch, index);
    MixParams p;
    p.j = (long)(((z2 & 0xFFFFFFFFull) * (unsigned long long)N) >> 32);
    const unsigned long long r = isqrt32((unsigned)(z2 >> 32));
    const int cx = (int)(((z3 & 0xFFFFull) * (unsigned long long)W) >> 16);
    const int cy = (int)((((z3 >> 16) & 0xFFFFull) * (unsigned long long)H) >> 16);
    p.apply = (unsigned)((z3 >> 32) & 0xFFFFull) < thresh ? 1 : 0;
    const int bw = (int)((r * (unsigned long long)W) >> 16);
    const int bh = (int)((r * (unsigned long long)H) >> 16);
    const int x0 = cx - bw / 2, y0 = cy - bh / 2;
    p.x0 = x0 < 0 ? 0 : x0;
    p.y0 = y0 < 0 ? 0 : y0;
    p.x1 = x0 + bw > W ? W : x0 + bw;
    p.y1 = y0 + bh > H ? H : y0 + bh;
    p.area = (p.x1 - p.x0) * (p.y1 - p.y0);     // <= H*W < 2^31
    return p;
}

template <int VEC>
__global__ __launch_bounds__(DATA_BLOCK)
void k_batch_gather_cutmix(const unsigned char* __restrict__ store,
                           const long* __restrict__ labels,
                           const long* __restrict__ index,
                           const unsigned short* __restrict__ lut,
                           unsigned short* __restrict__ out,
                           long* __restrict__ out_labels_a,
                           long* __restrict__ out_labels_b,
                           float* __restrict__ out_lam,
                           long N, long B, int H, int W, int C,
                           FastDiv divC, FastDiv divW,
                           unsigned chunks, unsigned tiles,
                           int pad, int hflip, unsigned thresh,
                           unsigned long long seed, unsigned long long epoch) {
    extern __shared__ unsigned short s_lut[];
    for (int i = threadIdx.x; i < C * 256; i += DATA_BLOCK) s_lut[i] = lut[i];
    __syncthreads();

    const int lane = threadIdx.x & (WAVE - 1);
    const long wave0 = (long)blockIdx.x * DATA_WAVES +
        __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long nwaves = (long)gridDim.x * DATA_WAVES;
    const long total = B * (long)tiles;
    const long E = (long)H * W * C;

    for (long t = wave0; t < total; t += nwaves) {
        const long b = t / tiles;                       // wave-uniform
        const unsigned tile = (unsigned)(t - b * tiles);
        long idx = index[b];
        idx = idx < 0 ? 0 : (idx >= N ? N - 1 : idx);   // documented clamp
        const MixParams mp = mix_decode(seed, epoch, (unsigned long long)idx,
                                        N, H, W, thresh);
        const long jdx = mp.apply ? mp.j : idx;         // in [0, N) either way
        const AugParams ai = aug_decode(seed, epoch, (unsigned long long)idx,
                                        pad, hflip);
        const AugParams aj = aug_decode(seed, epoch, (unsigned long long)jdx,
                                        pad, hflip);
        // not applied or empty: the box test below never fires
        const int bx0 = mp.apply ? mp.x0 : 0, bx1 = mp.apply ? mp.x1 : 0;
        const int by0 = mp.y0, by1 = mp.y1;
        if (tile == 0 && lane == 0) {
            const int HW = H * W;
            const int area = mp.apply ? mp.area : 0;
            out_labels_a[b] = labels[idx];
            out_labels_b[b] = labels[jdx];
            out_lam[b] = __fdiv_rn((float)(HW - area), (float)HW);
        }

        const unsigned k = tile * WAVE + lane;
        if (k >= chunks) continue;
        const unsigned e0 = k * VEC;
        const unsigned p0 = fd_div(e0, divC);
        int c = (int)fd_mod(e0, divC, p0);
        const unsigned y0 = fd_div(p0, divW);
        int x = (int)fd_mod(p0, divW, y0);
        int y = (int)y0;
        const unsigned char* src_i = store + idx * E;
        const unsigned char* src_j = store + jdx * E;
        const int oxi = ai.dx - pad, oyi = ai.dy - pad;
        const int oxj = aj.dx - pad, oyj = aj.dy - pad;

        unsigned short v[VEC];
        #pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const bool inbox = x >= bx0 && x < bx1 && y >= by0 && y < by1;
            const unsigned char* src = inbox ? src_j : src_i;
            const int flip = inbox ? aj.flip : ai.flip;
            const int sy = y + (inbox ? oyj : oyi);
            const int sx = (flip ? W - 1 - x : x) + (inbox ? oxj : oxi);
            const bool in = (unsigned)sy < (unsigned)H &&
                            (unsigned)sx < (unsigned)W;
            unsigned u = 0;
            if (in) u = src[(sy * W + sx) * C + c];   // < E < 2^31
            v[j] = s_lut[c * 256 + u];
            if (++c == C) {
                c = 0;
                if (++x == W) { x = 0; ++y; }
            }
        }
        unsigned short* dst = out + b * E + e0;
        if constexpr (VEC == 8) {
            s16x8 o;
            #pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (short)v[j];
            *reinterpret_cast<s16x8*>(dst) = o;
        } else {
            dst[0] = v[0];
        }
    }
}

std::vector<at::Tensor> batch_gather_cutmix(at::Tensor store, at::Tensor labels,
                                            at::Tensor index, at::Tensor lut,
                                            long pad, bool hflip, long seed,
                                            long epoch, long prob_thresh) {
    TORCH_CHECK(store.is_cuda() && store.scalar_type() == at::kByte &&
                store.dim() == 4 && store.is_contiguous(),
                "store must be a contiguous uint8 [N,H,W,C] device tensor");
    const long N = store.size(0);
    const long H = store.size(1), W = store.size(2), C = store.size(3);
    TORCH_CHECK(N >= 1 && N < (1ll << 32), "store needs 1 <= N < 2^32");
    TORCH_CHECK(H >= 1 && W >= 1 && C >= 1 && C <= DATA_MAX_C,
                "store needs H, W >= 1 and 1 <= C <= ", DATA_MAX_C);
    const long E = H * W * C;
    TORCH_CHECK(E < (1ll << 31), "sample too large");
    TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong &&
                labels.dim() == 1 && labels.size(0) == N &&
                labels.is_contiguous(), "labels must be int64 [N]");
    TORCH_CHECK(index.is_cuda() && index.scalar_type() == at::kLong &&
                index.dim() == 1 && index.is_contiguous(),
                "index must be a contiguous int64 [B] device tensor");
    TORCH_CHECK(lut.is_cuda() && lut.scalar_type() == at::kBFloat16 &&
                lut.dim() == 2 && lut.size(0) == C && lut.size(1) == 256 &&
                lut.is_contiguous(), "lut must be bf16 [C,256]");
    TORCH_CHECK(labels.device() == store.device() &&
                index.device() == store.device() &&
                lut.device() == store.device(),
                "all operands must live on one device");
    TORCH_CHECK(pad >= 0 && pad <= 4096, "pad must be in [0, 4096]");
    TORCH_CHECK(epoch >= 0 && epoch < (1ll << 32), "epoch must be in [0, 2^32)");
    TORCH_CHECK(prob_thresh >= 0 && prob_thresh <= 65536,
                "prob_thresh must be in [0, 65536]");

    const long B = index.size(0);
    auto images = at::empty(
        {B, C, H, W},
        store.options().dtype(at::kBFloat16)
            .memory_format(at::MemoryFormat::ChannelsLast));
    auto labels_a = at::empty({B}, labels.options());
    auto labels_b = at::empty({B}, labels.options());
    auto lam = at::empty({B}, store.options().dtype(at::kFloat));
    if (B == 0) return {images, labels_a, labels_b, lam};

    const bool vec = (E % 8) == 0;
    const unsigned chunks = (unsigned)(vec ? E / 8 : E);
    const unsigned tiles = (chunks + WAVE - 1) / WAVE;
    const long total = B * (long)tiles;
    const int blocks = (int)std::min<long>(
        DATA_MAX_BLOCKS, (total + DATA_WAVES - 1) / DATA_WAVES);
    FastDiv divC, divW;
    divC.init((unsigned)C);
    divW.init((unsigned)W);
    const size_t lds = (size_t)C * 256 * sizeof(unsigned short);
    auto stream = at::hip::getCurrentHIPStream();
    auto kern = vec ? k_batch_gather_cutmix<8> : k_batch_gather_cutmix<1>;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(DATA_BLOCK), lds,
                       stream.stream(), store.data_ptr<unsigned char>(),
                       labels.data_ptr<long>(), index.data_ptr<long>(),
                       reinterpret_cast<const unsigned short*>(lut.data_ptr()),
                       reinterpret_cast<unsigned short*>(images.data_ptr()),
                       labels_a.data_ptr<long>(), labels_b.data_ptr<long>(),
                       lam.data_ptr<float>(), N, B, (int)H, (int)W,
                       (int)C, divC, divW, chunks, tiles, (int)pad,
                       (int)hflip, (unsigned)prob_thresh,
                       (unsigned long long)seed, (unsigned long long)epoch);
    HIP_CHECK_LAST();
    return {images, labels_a, labels_b, lam};
}
