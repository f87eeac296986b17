// ce.hip — fused cross-entropy (log-softmax + NLL) fwd/bwd and the
// rowwise-argmax accuracy reduction.
//
// Row length is small (10 classes for the flagship config) so each thread
// owns one row; the loss mean over the batch is a deterministic two-stage
// reduction (per-block partials in fixed order, single-block combine) —
// no fp atomics.  Backward reads the upstream gradient from device memory
// (0-dim tensor) so no host sync is needed.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <climits>
#include "common.h"

constexpr int CE_BLOCK = 256;

// per-row: lse_i = log(sum exp(x - max)) + max ; rowloss_i = lse_i - x[t_i]
template <typename T>
__global__ void k_ce_rows(const T* __restrict__ logits,
                          const long* __restrict__ target,
                          float* __restrict__ rowloss,
                          float* __restrict__ lse_out,
                          int B, int C) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const T* row = logits + (long)i * C;
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, (float)row[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf((float)row[c] - mx);
    float lse = logf(s) + mx;
    lse_out[i] = lse;
    rowloss[i] = lse - (float)row[target[i]];
}

// Wave-per-row variants for wide rows (the ResNet-50 [B,1000] head —
// the thread-per-row kernel walks 3×C serially,
// 254 µs for ~4 MB of reads).  One 64-lane wave owns a row; lanes stream
// 16 B bf16x8 chunks (coalesced 1 KiB per wave-iteration) with an online
// softmax (single pass over the row), then a shfl tree combines the
// per-lane (max, scaled-sum) pairs.  bf16 rows with C % 8 == 0 only;
// everything else keeps the scalar kernels.
constexpr int CE_WPB = CE_BLOCK / WAVE;   // rows (waves) per block

DEV_INLINE void ce_online8(const s16x8 v, float& m, float& s) {
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
        float x = us2f((unsigned short)v[j]);
        if (x > m) {
            s *= expf(m - x);   // m == -inf ⇒ s == 0, exp(-inf)=0 handled
            m = x;
        }
        s += expf(x - m);
    }
}

__global__ void k_ce_rows_wave(const bf16* __restrict__ logits,
                               const long* __restrict__ target,
                               float* __restrict__ rowloss,
                               float* __restrict__ lse_out,
                               int B, int C) {
    const int row_i = blockIdx.x * CE_WPB + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row_i >= B) return;
    const bf16* row = logits + (long)row_i * C;
    const int chunks = C >> 3;
    float m = -INFINITY, s = 0.f;
    for (int ch = lane; ch < chunks; ch += WAVE) {
        s16x8 v = *reinterpret_cast<const s16x8*>(row + ch * 8);
        ce_online8(v, m, s);
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        float mo = __shfl_down(m, off, 64);
        float so = __shfl_down(s, off, 64);
        float mn = fmaxf(m, mo);
        float t1 = (s == 0.f) ? 0.f : s * expf(m - mn);
        float t2 = (so == 0.f) ? 0.f : so * expf(mo - mn);
        m = mn;
        s = t1 + t2;
    }
    if (lane == 0) {
        float lse = logf(s) + m;
        lse_out[row_i] = lse;
        rowloss[row_i] = lse - (float)row[target[row_i]];
    }
}

__global__ void k_ce_bwd_wave(const bf16* __restrict__ logits,
                              const long* __restrict__ target,
                              const float* __restrict__ lse,
                              const float* __restrict__ dloss,
                              bf16* __restrict__ dlogits, int B, int C) {
    const int row_i = blockIdx.x * CE_WPB + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row_i >= B) return;
    const float g = dloss[0] / B;
    const bf16* row = logits + (long)row_i * C;
    bf16* drow = dlogits + (long)row_i * C;
    const float l = lse[row_i];
    const int t = (int)target[row_i];
    const int chunks = C >> 3;
    for (int ch = lane; ch < chunks; ch += WAVE) {
        s16x8 v = *reinterpret_cast<const s16x8*>(row + ch * 8);
        s16x8 o;
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
            int c = ch * 8 + j;
            float p = expf(us2f((unsigned short)v[j]) - l);
            o[j] = (short)f2us((p - (c == t ? 1.f : 0.f)) * g);
        }
        *reinterpret_cast<s16x8*>(drow + ch * 8) = o;
    }
}

__global__ void k_argmax_correct_wave(const bf16* __restrict__ logits,
                                      const long* __restrict__ target,
                                      long long* __restrict__ out,
                                      int B, int C) {
    const int row_i = blockIdx.x * CE_WPB + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row_i >= B) return;
    const bf16* row = logits + (long)row_i * C;
    const int chunks = C >> 3;
    float best = -INFINITY;
    int arg = INT_MAX;
    for (int ch = lane; ch < chunks; ch += WAVE) {
        s16x8 v = *reinterpret_cast<const s16x8*>(row + ch * 8);
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
            float x = us2f((unsigned short)v[j]);
            if (x > best) { best = x; arg = ch * 8 + j; }
        }
    }
    // combine with torch's first-max tie rule: larger value wins, equal
    // value ⇒ smaller index wins
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        float bo = __shfl_down(best, off, 64);
        int ao = __shfl_down(arg, off, 64);
        if (bo > best || (bo == best && ao < arg)) { best = bo; arg = ao; }
    }
    if (lane == 0 && arg == (int)target[row_i])
        atomicAdd(reinterpret_cast<unsigned long long*>(out), 1ull);
}

static inline bool ce_wave_ok(const at::Tensor& logits, int C) {
    return logits.scalar_type() == at::kBFloat16 && (C % 8) == 0 && C >= 64;
}

// deterministic mean: single block, fixed-order tree over per-thread partials
__global__ void k_reduce_mean(const float* __restrict__ rowloss, int B,
                              float* __restrict__ out) {
    __shared__ float partial[CE_BLOCK];
    float acc = 0.f;
    for (int i = threadIdx.x; i < B; i += CE_BLOCK) acc += rowloss[i];
    partial[threadIdx.x] = acc;
    __syncthreads();
    for (int off = CE_BLOCK / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) partial[threadIdx.x] += partial[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = partial[0] / B;
}

std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor target) {
    TORCH_CHECK(logits.dim() == 2 && logits.is_cuda() && logits.is_contiguous());
    TORCH_CHECK(target.scalar_type() == at::kLong);
    int B = logits.size(0), C = logits.size(1);
    auto opts = logits.options().dtype(at::kFloat);
    auto rowloss = at::empty({B}, opts);
    auto lse = at::empty({B}, opts);
    auto loss = at::empty({}, opts);
    auto stream = at::hip::getCurrentHIPStream();
    int blocks = ceil_div_i(B, CE_BLOCK);
    if (ce_wave_ok(logits, C)) {
        hipLaunchKernelGGL(k_ce_rows_wave, dim3(ceil_div_i(B, CE_WPB)),
                           dim3(CE_BLOCK), 0, stream.stream(),
                           reinterpret_cast<const bf16*>(logits.data_ptr()),
                           target.data_ptr<long>(), rowloss.data_ptr<float>(),
                           lse.data_ptr<float>(), B, C);
    } else if (logits.scalar_type() == at::kBFloat16) {
        hipLaunchKernelGGL(k_ce_rows<bf16>, dim3(blocks), dim3(CE_BLOCK), 0,
                           stream.stream(),
                           reinterpret_cast<const bf16*>(logits.data_ptr()),
                           target.data_ptr<long>(), rowloss.data_ptr<float>(),
                           lse.data_ptr<float>(), B, C);
    } else {
        TORCH_CHECK(logits.scalar_type() == at::kFloat);
        hipLaunchKernelGGL(k_ce_rows<float>, dim3(blocks), dim3(CE_BLOCK), 0,
                           stream.stream(), logits.data_ptr<float>(),
                           target.data_ptr<long>(), rowloss.data_ptr<float>(),
                           lse.data_ptr<float>(), B, C);
    }
    HIP_CHECK_LAST();
    hipLaunchKernelGGL(k_reduce_mean, dim3(1), dim3(CE_BLOCK), 0,
                       stream.stream(), rowloss.data_ptr<float>(),
                       B, loss.data_ptr<float>());
    HIP_CHECK_LAST();
    return {loss, lse};
}

// dlogits[i,c] = (softmax(i,c) - [c==t_i]) * (*dloss) / B
template <typename T>
__global__ void k_ce_bwd(const T* __restrict__ logits,
                         const long* __restrict__ target,
                         const float* __restrict__ lse,
                         const float* __restrict__ dloss,
                         T* __restrict__ dlogits, int B, int C) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    float g = dloss[0] / B;
    const T* row = logits + (long)i * C;
    T* drow = dlogits + (long)i * C;
    float l = lse[i];
    long t = target[i];
    for (int c = 0; c < C; ++c) {
        float p = expf((float)row[c] - l);
        drow[c] = (T)((p - (c == t ? 1.f : 0.f)) * g);
    }
}

at::Tensor ce_bwd(at::Tensor logits, at::Tensor target, at::Tensor lse,
                  at::Tensor dloss) {
    int B = logits.size(0), C = logits.size(1);
    auto dlogits = at::empty_like(logits);
    auto stream = at::hip::getCurrentHIPStream();
    int blocks = ceil_div_i(B, CE_BLOCK);
    auto dlossf = dloss.scalar_type() == at::kFloat ? dloss : dloss.to(at::kFloat);
    if (ce_wave_ok(logits, C)) {
        hipLaunchKernelGGL(k_ce_bwd_wave, dim3(ceil_div_i(B, CE_WPB)),
                           dim3(CE_BLOCK), 0, stream.stream(),
                           reinterpret_cast<const bf16*>(logits.data_ptr()),
                           target.data_ptr<long>(), lse.data_ptr<float>(),
                           dlossf.data_ptr<float>(),
                           reinterpret_cast<bf16*>(dlogits.data_ptr()), B, C);
    } else if (logits.scalar_type() == at::kBFloat16) {
        hipLaunchKernelGGL(k_ce_bwd<bf16>, dim3(blocks), dim3(CE_BLOCK), 0,
                           stream.stream(),
                           reinterpret_cast<const bf16*>(logits.data_ptr()),
                           target.data_ptr<long>(), lse.data_ptr<float>(),
                           dlossf.data_ptr<float>(),
                           reinterpret_cast<bf16*>(dlogits.data_ptr()), B, C);
    } else {
        hipLaunchKernelGGL(k_ce_bwd<float>, dim3(blocks), dim3(CE_BLOCK), 0,
                           stream.stream(), logits.data_ptr<float>(),
                           target.data_ptr<long>(), lse.data_ptr<float>(),
                           dlossf.data_ptr<float>(),
                           dlogits.data_ptr<float>(), B, C);
    }
    HIP_CHECK_LAST();
    return dlogits;
}

// ------------------------------------------------------- argmax + correct ---

// first-max-index argmax per row (torch CPU tie semantics), compare with
// target, deterministic integer block+atomic accumulation.
template <typename T>
__global__ void k_argmax_correct(const T* __restrict__ logits,
                                 const long* __restrict__ target,
                                 long long* __restrict__ out, int B, int C) {
    __shared__ long long scratch[CE_BLOCK / WAVE];
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    long long correct = 0;
    if (i < B) {
        const T* row = logits + (long)i * C;
        float best = (float)row[0];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            float v = (float)row[c];
            if (v > best) { best = v; arg = c; }
        }
        correct = (arg == (int)target[i]) ? 1 : 0;
    }
    long long total = lds_block_reduce_ll(correct, scratch);
    if (threadIdx.x == 0 && total)
        atomicAdd(reinterpret_cast<unsigned long long*>(out),
                  (unsigned long long)total);
}

at::Tensor argmax_correct(at::Tensor logits, at::Tensor target) {
    TORCH_CHECK(logits.dim() == 2 && logits.is_cuda());
    auto lc = logits.contiguous();
    int B = lc.size(0), C = lc.size(1);
    auto out = at::zeros({}, lc.options().dtype(at::kLong));
    auto stream = at::hip::getCurrentHIPStream();
    int blocks = ceil_div_i(B, CE_BLOCK);
    if (ce_wave_ok(lc, C)) {
        hipLaunchKernelGGL(k_argmax_correct_wave, dim3(ceil_div_i(B, CE_WPB)),
                           dim3(CE_BLOCK), 0, stream.stream(),
                           reinterpret_cast<const bf16*>(lc.data_ptr()),
                           target.data_ptr<long>(),
                           reinterpret_cast<long long*>(out.data_ptr()), B, C);
    } else if (lc.scalar_type() == at::kBFloat16) {
        hipLaunchKernelGGL(k_argmax_correct<bf16>, dim3(blocks), dim3(CE_BLOCK),
                           0, stream.stream(),
                           reinterpret_cast<const bf16*>(lc.data_ptr()),
                           target.data_ptr<long>(),
                           reinterpret_cast<long long*>(out.data_ptr()), B, C);
    } else {
        hipLaunchKernelGGL(k_argmax_correct<float>, dim3(blocks), dim3(CE_BLOCK),
                           0, stream.stream(), lc.data_ptr<float>(),
                           target.data_ptr<long>(),
                           reinterpret_cast<long long*>(out.data_ptr()), B, C);
    }
    HIP_CHECK_LAST();
    return out;
}

// ------------------------------------------- mixed-target, smoothed CE ------
//
// Cross-entropy against the target distribution
//     q_i = eps/C + (1-eps) * (lam_i * onehot(a_i) + (1-lam_i) * onehot(b_i))
// (label smoothing: b = a, lam = 1; CutMix / mixup: a target pair with a
// per-row weight).  Per row
//     rowloss_i = lse_i - [(1-eps) * (lam_i*x[a_i] + (1-lam_i)*x[b_i])
//                          + (eps/C) * sum_c x[i,c]]
//     dlogits[i,c] = (softmax(i,c) - q_i[c]) * (*dloss) / B
// The one-hots ADD, so a == b carries the weight lam + (1-lam) once.
// sum_c x rides in the pass that already walks the row: one more running
// sum next to the maximum in the thread-per-row kernel, one more
// accumulator (8-element pairwise tree per chunk) and one more shuffle tree
// in the wave-per-row kernel.  The plain kernels above are untouched; these
// are separate kernels so the hard-target path stays the hard-target path.
// The fp32 operation order below is what tests/test_gpu_ce_mix.py counts.

struct CeMixRow {
    float qa, qb;   // (1-eps)*lam, (1-eps)*(1-lam)
};

DEV_INLINE float ce_mix_pick(float xa, float xb, float lam, float sx,
                             float om, float ec) {
    const float tsel = lam * xa + (1.f - lam) * xb;
    // ec == 0 (no smoothing) must not turn an overflowed row sum into a NaN
    const float smooth = (ec != 0.f) ? ec * sx : 0.f;
    return om * tsel + smooth;
}

DEV_INLINE CeMixRow ce_mix_q(float lam, float om) {
    CeMixRow r;
    r.qa = om * lam;
    r.qb = om * (1.f - lam);
    return r;
}

template <typename T>
__global__ void k_ce_mix_rows(const T* __restrict__ logits,
                              const long* __restrict__ ta,
                              const long* __restrict__ tb,
                              const float* __restrict__ lam,
                              float* __restrict__ rowloss,
                              float* __restrict__ lse_out,
                              int B, int C, float om, float ec) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const T* row = logits + (long)i * C;
    float mx = -INFINITY, sx = 0.f;
    for (int c = 0; c < C; ++c) {
        const float x = (float)row[c];
        mx = fmaxf(mx, x);
        sx += x;
    }
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf((float)row[c] - mx);
    float lse = logf(s) + mx;
    lse_out[i] = lse;
    rowloss[i] = lse - ce_mix_pick((float)row[ta[i]], (float)row[tb[i]],
                                   lam[i], sx, om, ec);
}

__global__ void k_ce_mix_rows_wave(const bf16* __restrict__ logits,
                                   const long* __restrict__ ta,
                                   const long* __restrict__ tb,
                                   const float* __restrict__ lam,
                                   float* __restrict__ rowloss,
                                   float* __restrict__ lse_out,
                                   int B, int C, float om, float ec) {
    const int row_i = blockIdx.x * CE_WPB + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row_i >= B) return;
    const bf16* row = logits + (long)row_i * C;
    const int chunks = C >> 3;
    float m = -INFINITY, s = 0.f, sx = 0.f;
    for (int ch = lane; ch < chunks; ch += WAVE) {
        s16x8 v = *reinterpret_cast<const s16x8*>(row + ch * 8);
        ce_online8(v, m, s);
        const float x01 = us2f((unsigned short)v[0]) + us2f((unsigned short)v[1]);
        const float x23 = us2f((unsigned short)v[2]) + us2f((unsigned short)v[3]);
        const float x45 = us2f((unsigned short)v[4]) + us2f((unsigned short)v[5]);
        const float x67 = us2f((unsigned short)v[6]) + us2f((unsigned short)v[7]);
        sx += (x01 + x23) + (x45 + x67);
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        float mo = __shfl_down(m, off, 64);
        float so = __shfl_down(s, off, 64);
        float mn = fmaxf(m, mo);
        float t1 = (s == 0.f) ? 0.f : s * expf(m - mn);
        float t2 = (so == 0.f) ? 0.f : so * expf(mo - mn);
        m = mn;
        s = t1 + t2;
        sx += __shfl_down(sx, off, 64);
    }
    if (lane == 0) {
        float lse = logf(s) + m;
        lse_out[row_i] = lse;
        rowloss[row_i] = lse - ce_mix_pick((float)row[ta[row_i]],
                                           (float)row[tb[row_i]],
                                           lam[row_i], sx, om, ec);
    }
}

template <typename T>
__global__ void k_ce_mix_bwd(const T* __restrict__ logits,
                             const long* __restrict__ ta,
                             const long* __restrict__ tb,
                             const float* __restrict__ lam,
                             const float* __restrict__ lse,
                             const float* __restrict__ dloss,
                             T* __restrict__ dlogits, int B, int C,
                             float om, float ec) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    float g = dloss[0] / B;
    const T* row = logits + (long)i * C;
    T* drow = dlogits + (long)i * C;
    float l = lse[i];
    const long a = ta[i], b = tb[i];
    const CeMixRow qr = ce_mix_q(lam[i], om);
    for (int c = 0; c < C; ++c) {
        float p = expf((float)row[c] - l);
        float q = ec + (c == a ? qr.qa : 0.f) + (c == b ? qr.qb : 0.f);
        drow[c] = (T)((p - q) * g);
    }
}

__global__ void k_ce_mix_bwd_wave(const bf16* __restrict__ logits,
                                  const long* __restrict__ ta,
                                  const long* __restrict__ tb,
                                  const float* __restrict__ lam,
                                  const float* __restrict__ lse,
                                  const float* __restrict__ dloss,
                                  bf16* __restrict__ dlogits, int B, int C,
                                  float om, float ec) {
    const int row_i = blockIdx.x * CE_WPB + ((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row_i >= B) return;
    const float g = dloss[0] / B;
    const bf16* row = logits + (long)row_i * C;
    bf16* drow = dlogits + (long)row_i * C;
    const float l = lse[row_i];
    const int a = (int)ta[row_i], b = (int)tb[row_i];
    const CeMixRow qr = ce_mix_q(lam[row_i], om);
    const int chunks = C >> 3;
    for (int ch = lane; ch < chunks; ch += WAVE) {
        s16x8 v = *reinterpret_cast<const s16x8*>(row + ch * 8);
        s16x8 o;
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
            int c = ch * 8 + j;
            float p = expf(us2f((unsigned short)v[j]) - l);
            float q = ec + (c == a ? qr.qa : 0.f) + (c == b ? qr.qb : 0.f);
            o[j] = (short)f2us((p - q) * g);
        }
        *reinterpret_cast<s16x8*>(drow + ch * 8) = o;
    }
}

// host-side operand checks (metadata only: no device sync)
static void ce_mix_check(const at::Tensor& logits, const at::Tensor& ta,
                         const at::Tensor& tb, const at::Tensor& lam,
                         double smoothing) {
    TORCH_CHECK(logits.dim() == 2 && logits.is_cuda() && logits.is_contiguous(),
                "logits must be a contiguous [B,C] device tensor");
    TORCH_CHECK(logits.scalar_type() == at::kBFloat16 ||
                logits.scalar_type() == at::kFloat,
                "logits must be bf16 or fp32");
    const long B = logits.size(0);
    TORCH_CHECK(logits.size(1) >= 1, "logits need at least one class");
    TORCH_CHECK(ta.scalar_type() == at::kLong && tb.scalar_type() == at::kLong,
                "target_a and target_b must be int64");
    TORCH_CHECK(lam.scalar_type() == at::kFloat, "lam must be fp32");
    TORCH_CHECK(ta.dim() == 1 && ta.size(0) == B && ta.is_contiguous() &&
                tb.dim() == 1 && tb.size(0) == B && tb.is_contiguous() &&
                lam.dim() == 1 && lam.size(0) == B && lam.is_contiguous(),
                "target_a, target_b and lam must be contiguous [B]");
    TORCH_CHECK(ta.device() == logits.device() &&
                tb.device() == logits.device() &&
                lam.device() == logits.device(),
                "target_a, target_b and lam must live on the logits' device");
    TORCH_CHECK(smoothing >= 0.0 && smoothing < 1.0,
                "smoothing must be in [0, 1), got ", smoothing);
}

std::vector<at::Tensor> ce_mix_fwd(at::Tensor logits, at::Tensor target_a,
                                   at::Tensor target_b, at::Tensor lam,
                                   double smoothing) {
    ce_mix_check(logits, target_a, target_b, lam, smoothing);
    int B = logits.size(0), C = logits.size(1);
    const float eps = (float)smoothing;
    const float om = 1.f - eps, ec = eps / (float)C;
    auto opts = logits.options().dtype(at::kFloat);
    auto rowloss = at::empty({B}, opts);
    auto lse = at::empty({B}, opts);
    auto loss = at::empty({}, opts);
    if (B == 0) return {loss.fill_(NAN), lse};
    auto stream = at::hip::getCurrentHIPStream();
    int blocks = ceil_div_i(B, CE_BLOCK);
    if (ce_wave_ok(logits, C)) {
        hipLaunchKernelGGL(k_ce_mix_rows_wave, dim3(ceil_div_i(B, CE_WPB)),
                           dim3(CE_BLOCK), 0, stream.stream(),
                           reinterpret_cast<const bf16*>(logits.data_ptr()),
                           target_a.data_ptr<long>(), target_b.data_ptr<long>(),
                           lam.data_ptr<float>(), rowloss.data_ptr<float>(),
                           lse.data_ptr<float>(), B, C, om, ec);
    } else if (logits.scalar_type() == at::kBFloat16) {
        hipLaunchKernelGGL(k_ce_mix_rows<bf16>, dim3(blocks), dim3(CE_BLOCK), 0,
                           stream.stream(),
                           reinterpret_cast<const bf16*>(logits.data_ptr()),
                           target_a.data_ptr<long>(), target_b.data_ptr<long>(),
                           lam.data_ptr<float>(), rowloss.data_ptr<float>(),
                           lse.data_ptr<float>(), B, C, om, ec);
    } else {
        hipLaunchKernelGGL(k_ce_mix_rows<float>, dim3(blocks), dim3(CE_BLOCK), 0,
                           stream.stream(), logits.data_ptr<float>(),
                           target_a.data_ptr<long>(), target_b.data_ptr<long>(),
                           lam.data_ptr<float>(), rowloss.data_ptr<float>(),
                           lse.data_ptr<float>(), B, C, om, ec);
    }
    HIP_CHECK_LAST();
    hipLaunchKernelGGL(k_reduce_mean, dim3(1), dim3(CE_BLOCK), 0,
                       stream.stream(), rowloss.data_ptr<float>(),
                       B, loss.data_ptr<float>());
    HIP_CHECK_LAST();
    return {loss, lse};
}

at::Tensor ce_mix_bwd(at::Tensor logits, at::Tensor target_a,
                      at::Tensor target_b, at::Tensor lam, at::Tensor lse,
                      at::Tensor dloss, double smoothing) {
    ce_mix_check(logits, target_a, target_b, lam, smoothing);
    int B = logits.size(0), C = logits.size(1);
    TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.dim() == 1 &&
                lse.size(0) == B && lse.is_contiguous() &&
                lse.device() == logits.device(), "lse must be fp32 [B]");
    TORCH_CHECK(dloss.numel() == 1 && dloss.device() == logits.device(),
                "dloss must be a one-element device tensor");
    const float eps = (float)smoothing;
    const float om = 1.f - eps, ec = eps / (float)C;
    auto dlogits = at::empty_like(logits);
    if (B == 0) return dlogits;
    auto stream = at::hip::getCurrentHIPStream();
    int blocks = ceil_div_i(B, CE_BLOCK);
    auto dlossf = dloss.scalar_type() == at::kFloat ? dloss : dloss.to(at::kFloat);
    if (ce_wave_ok(logits, C)) {
        hipLaunchKernelGGL(k_ce_mix_bwd_wave, dim3(ceil_div_i(B, CE_WPB)),
                           dim3(CE_BLOCK), 0, stream.stream(),
                           reinterpret_cast<const bf16*>(logits.data_ptr()),
                           target_a.data_ptr<long>(), target_b.data_ptr<long>(),
                           lam.data_ptr<float>(), lse.data_ptr<float>(),
                           dlossf.data_ptr<float>(),
                           reinterpret_cast<bf16*>(dlogits.data_ptr()), B, C,
                           om, ec);
    } else if (logits.scalar_type() == at::kBFloat16) {
        hipLaunchKernelGGL(k_ce_mix_bwd<bf16>, dim3(blocks), dim3(CE_BLOCK), 0,
                           stream.stream(),
                           reinterpret_cast<const bf16*>(logits.data_ptr()),
                           target_a.data_ptr<long>(), target_b.data_ptr<long>(),
                           lam.data_ptr<float>(), lse.data_ptr<float>(),
                           dlossf.data_ptr<float>(),
                           reinterpret_cast<bf16*>(dlogits.data_ptr()), B, C,
                           om, ec);
    } else {
        hipLaunchKernelGGL(k_ce_mix_bwd<float>, dim3(blocks), dim3(CE_BLOCK), 0,
                           stream.stream(), logits.data_ptr<float>(),
                           target_a.data_ptr<long>(), target_b.data_ptr<long>(),
                           lam.data_ptr<float>(), lse.data_ptr<float>(),
                           dlossf.data_ptr<float>(),
                           dlogits.data_ptr<float>(), B, C, om, ec);
    }
    HIP_CHECK_LAST();
    return dlogits;
}
