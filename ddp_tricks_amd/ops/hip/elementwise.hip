// elementwise.hip — multi-tensor optimizer/amp kernels + casts.
//
// Implements the implicit native surface of apex amp_C + the fused SGD step
// (SURVEY N4/N12/N13): multi-tensor unscale+inf-check over the DDP bucket
// flats, fused SGD(momentum, nesterov) [+ Lookahead interpolation] over the
// whole parameter list in one launch, bf16<->fp32 casts.  Global grad-norm
// clipping rides on the same two passes: per-chunk sums of squares out of
// the unscale kernel, a one-block finalize (norm + clip coefficient, on
// device), and the coefficient applied inside the SGD's gradient read.
// Fused LARS adds per-tensor reductions on the same (tensor, chunk) scheme:
// pair square sums, a per-tensor trust ratio, and the SGD body with it.
// Fused AdamW and LAMB add a device-side step counter (k_mt_adam_tick), so
// that an overflow-skipped step does not advance the bias correction.
//
// Multi-tensor scheme: host packs up to MT_MAX tensor pointers + a prefix
// of chunk offsets into the kernarg struct; blocks map to (tensor, chunk)
// so one launch covers the whole list.  16 Ki-element chunks give ≳350
// blocks on the 23 MB flagship parameter set (256-CU chip wants ≫256
// workgroups); bodies are f32x4-vectorized.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

#include <vector>

constexpr int MT_MAX = 32;
constexpr int MT_CHUNK = 1 << 14;  // elements per block-chunk
constexpr int MT_BLOCK = 256;

struct MTMeta {
    const float* __restrict__ a[MT_MAX];
    float* __restrict__ b[MT_MAX];
    float* __restrict__ c[MT_MAX];
    long sizes[MT_MAX];
    int chunk_start[MT_MAX + 1];  // prefix sum of per-tensor chunk counts
    int ntensors;
};

DEV_INLINE int find_tensor(const MTMeta& m, int chunk, int& local_chunk) {
    int t = 0;
    while (t + 1 < m.ntensors && m.chunk_start[t + 1] <= chunk) ++t;
    local_chunk = chunk - m.chunk_start[t];
    return t;
}

DEV_INLINE void chunk_range(const MTMeta& m, int& t, long& base, long& end) {
    int local;
    t = find_tensor(m, blockIdx.x, local);
    long n = m.sizes[t];
    base = (long)local * MT_CHUNK;
    end = base + MT_CHUNK < n ? base + MT_CHUNK : n;
}

// ---------------------------------------------------------------- unscale ---

// Fixed-order block sum (MT_BLOCK threads): 64-lane wave shuffles, then an
// LDS tree over the per-wave partials.  No atomics — same inputs, same bits
// (the bn.hip split-reduction contract).  Result valid in thread 0.
DEV_INLINE float mt_block_sum(float v) {
    __shared__ float red[MT_BLOCK / WAVE];
    v = wave_reduce_sum(v);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    #pragma unroll
    for (int s = MT_BLOCK / WAVE / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// One (tensor, chunk) pass shared by the unscale and square-sum kernels.
// SCALE: g *= inv_scale in place + non-finite check (the amp unscale).
// NORM:  per-thread fp32 sum of squares of the values written (SCALE) or
//        read (!SCALE); the element->thread mapping and the accumulation
//        order are the same either way, so the fused and the read-only
//        kernels give bitwise-identical partials on identical contents.
template <bool SCALE, bool NORM>
DEV_INLINE void mt_chunk_pass(float* g, long base, long end, float inv_scale,
                              bool& bad, float& acc) {
    long vb = base >> 2, ve = end >> 2;
    for (long i = vb + threadIdx.x; i < ve; i += MT_BLOCK) {
        f32x4 v = reinterpret_cast<f32x4*>(g)[i];
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (SCALE) {
                v[j] *= inv_scale;
                if (!isfinite(v[j])) bad = true;
            }
            if (NORM) acc = fmaf(v[j], v[j], acc);
        }
        if (SCALE) reinterpret_cast<f32x4*>(g)[i] = v;
    }
    for (long i = ve * 4 + threadIdx.x; i < end; i += MT_BLOCK) {
        float v = g[i];
        if (SCALE) {
            v *= inv_scale;
            if (!isfinite(v)) bad = true;
            g[i] = v;
        }
        if (NORM) acc = fmaf(v, v, acc);
    }
}

// NORM=false is the plain amp unscale.  NORM=true also writes the chunk's
// sum of squares (of the unscaled values) to partials[chunk_base+blockIdx.x];
// chunk_base = chunks of earlier MT_MAX launch groups, so the partial index
// is global over the whole tensor list.
template <bool NORM>
__global__ void k_mt_unscale(MTMeta m, float inv_scale, float* found_inf,
                             float* __restrict__ partials, int chunk_base) {
    int t; long base, end;
    chunk_range(m, t, base, end);
    bool bad = false;
    float acc = 0.f;
    mt_chunk_pass<true, NORM>(m.b[t], base, end, inv_scale, bad, acc);
    if (bad) *found_inf = 1.0f;  // racy same-value store: any writer sets it
    if (NORM) {
        float s = mt_block_sum(acc);
        if (threadIdx.x == 0) partials[chunk_base + blockIdx.x] = s;
    }
}

// Read-only square-sum with the same partial layout (non-amp path and the
// standalone clip_grad_norm_).
__global__ void k_mt_sqsum(MTMeta m, float* __restrict__ partials,
                           int chunk_base) {
    int t; long base, end;
    chunk_range(m, t, base, end);
    bool bad = false;
    float acc = 0.f;
    mt_chunk_pass<false, true>(m.b[t], base, end, 1.0f, bad, acc);
    float s = mt_block_sum(acc);
    if (threadIdx.x == 0) partials[chunk_base + blockIdx.x] = s;
}

static int mt_total_chunks(const std::vector<at::Tensor>& ts) {
    long total = 0;
    for (auto& t : ts) total += ceil_div_i(t.numel(), MT_CHUNK);
    TORCH_CHECK(total < (1L << 31), "multi-tensor list too large");
    return (int)total;
}

static float* mt_check_partials(const at::Tensor& partials, int total) {
    TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == at::kFloat &&
                partials.is_contiguous(), "partials: contiguous cuda fp32");
    TORCH_CHECK(partials.numel() >= total, "partials holds ",
                partials.numel(), " floats, need ", total, " (one per chunk)");
    return partials.data_ptr<float>();
}

long mt_chunk_elems() { return MT_CHUNK; }

void multi_tensor_unscale(std::vector<at::Tensor> grads, at::Tensor found_inf,
                          double inv_scale,
                          c10::optional<at::Tensor> partials) {
    auto stream = at::hip::getCurrentHIPStream();
    float* pp = nullptr;
    if (partials.has_value())
        pp = mt_check_partials(*partials, mt_total_chunks(grads));
    int chunk_base = 0;
    for (size_t start = 0; start < grads.size(); start += MT_MAX) {
        MTMeta m{};
        int chunks = 0;
        int nt = 0;
        for (size_t i = start; i < std::min(grads.size(), start + MT_MAX); ++i) {
            auto& g = grads[i];
            TORCH_CHECK(g.is_cuda() && g.scalar_type() == at::kFloat &&
                        g.is_contiguous(), "unscale expects contiguous fp32");
            m.b[nt] = g.data_ptr<float>();
            m.sizes[nt] = g.numel();
            m.chunk_start[nt] = chunks;
            chunks += ceil_div_i(g.numel(), MT_CHUNK);
            ++nt;
        }
        m.chunk_start[nt] = chunks;
        m.ntensors = nt;
        if (chunks == 0) continue;
        if (pp)
            hipLaunchKernelGGL(k_mt_unscale<true>, dim3(chunks),
                               dim3(MT_BLOCK), 0, stream.stream(), m,
                               (float)inv_scale, found_inf.data_ptr<float>(),
                               pp, chunk_base);
        else
            hipLaunchKernelGGL(k_mt_unscale<false>, dim3(chunks),
                               dim3(MT_BLOCK), 0, stream.stream(), m,
                               (float)inv_scale, found_inf.data_ptr<float>(),
                               (float*)nullptr, 0);
        HIP_CHECK_LAST();
        chunk_base += chunks;
    }
}

void multi_tensor_sqsum(std::vector<at::Tensor> tensors, at::Tensor partials) {
    auto stream = at::hip::getCurrentHIPStream();
    float* pp = mt_check_partials(partials, mt_total_chunks(tensors));
    int chunk_base = 0;
    for (size_t start = 0; start < tensors.size(); start += MT_MAX) {
        MTMeta m{};
        int chunks = 0, nt = 0;
        for (size_t i = start; i < std::min(tensors.size(), start + MT_MAX); ++i) {
            auto& g = tensors[i];
            TORCH_CHECK(g.is_cuda() && g.scalar_type() == at::kFloat &&
                        g.is_contiguous(), "sqsum expects contiguous fp32");
            m.b[nt] = g.data_ptr<float>();
            m.sizes[nt] = g.numel();
            m.chunk_start[nt] = chunks;
            chunks += ceil_div_i(g.numel(), MT_CHUNK);
            ++nt;
        }
        m.chunk_start[nt] = chunks;
        m.ntensors = nt;
        if (chunks == 0) continue;
        hipLaunchKernelGGL(k_mt_sqsum, dim3(chunks), dim3(MT_BLOCK), 0,
                           stream.stream(), m, pp, chunk_base);
        HIP_CHECK_LAST();
        chunk_base += chunks;
    }
}

// ---------------------------------------------------- norm finalize / clip ---

// One block: norm = sqrt(sum of the n chunk partials), summed in double in a
// fixed order (thread i takes partials i, i+256, ...; then a fixed LDS tree).
//   out[0] = norm
//   out[1] = clip coefficient = min(1, max_norm / (norm + 1e-6)), torch's
//            clip_grad_norm_ formula; 1.0 when clipping is off, the norm is
//            non-finite or found_inf is set (that step is skipped device-side
//            anyway, and the coefficient must never be NaN).
//   stats (optional) = {sum of finite norms, max finite norm,
//                       #steps with coef < 1, #finite steps}.
__global__ void k_mt_norm_finalize(const float* __restrict__ partials, int n,
                                   float max_norm,
                                   const float* __restrict__ found_inf,
                                   float* __restrict__ out,
                                   float* __restrict__ stats) {
    __shared__ double red[MT_BLOCK];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += MT_BLOCK) s += (double)partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    #pragma unroll
    for (int w = MT_BLOCK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    float norm = (float)sqrt(red[0]);
    bool ok = isfinite(norm) && !(found_inf && *found_inf != 0.0f);
    float coef = 1.0f;
    if (ok && max_norm > 0.0f)
        coef = fminf(1.0f, __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f)));
    out[0] = norm;
    out[1] = coef;
    if (stats && ok) {
        stats[0] += norm;
        stats[1] = fmaxf(stats[1], norm);
        if (coef < 1.0f) stats[2] += 1.0f;
        stats[3] += 1.0f;
    }
}

void norm_finalize(at::Tensor partials, long n, double max_norm,
                   c10::optional<at::Tensor> found_inf, at::Tensor out,
                   c10::optional<at::Tensor> stats) {
    TORCH_CHECK(n >= 0 && n < (1L << 31));
    float* pp = mt_check_partials(partials, (int)n);
    TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat &&
                out.is_contiguous() && out.numel() >= 2,
                "norm_finalize: out must be >=2 contiguous cuda fp32");
    float* sp = nullptr;
    if (stats.has_value()) {
        TORCH_CHECK(stats->is_cuda() && stats->scalar_type() == at::kFloat &&
                    stats->is_contiguous() && stats->numel() >= 4,
                    "norm_finalize: stats must be >=4 contiguous cuda fp32");
        sp = stats->data_ptr<float>();
    }
    const float* fi = found_inf.has_value()
        ? found_inf->data_ptr<float>() : nullptr;
    auto stream = at::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(k_mt_norm_finalize, dim3(1), dim3(MT_BLOCK), 0,
                       stream.stream(), pp, (int)n, (float)max_norm, fi,
                       out.data_ptr<float>(), sp);
    HIP_CHECK_LAST();
}

// g *= *coef in place (the non-lazy clip); no-op when found_inf is set.
__global__ void k_mt_scale(MTMeta m, const float* __restrict__ coef,
                           const float* __restrict__ found_inf) {
    if (found_inf && *found_inf != 0.0f) return;
    const float c = *coef;
    int t; long base, end;
    chunk_range(m, t, base, end);
    float* g = m.b[t];
    long vb = base >> 2, ve = end >> 2;
    for (long i = vb + threadIdx.x; i < ve; i += MT_BLOCK) {
        f32x4 v = reinterpret_cast<f32x4*>(g)[i];
        #pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __fmul_rn(v[j], c);
        reinterpret_cast<f32x4*>(g)[i] = v;
    }
    for (long i = ve * 4 + threadIdx.x; i < end; i += MT_BLOCK)
        g[i] = __fmul_rn(g[i], c);
}

void multi_tensor_scale(std::vector<at::Tensor> tensors, at::Tensor coef,
                        c10::optional<at::Tensor> found_inf) {
    TORCH_CHECK(coef.is_cuda() && coef.scalar_type() == at::kFloat &&
                coef.numel() >= 1, "scale: coef must be a cuda fp32 tensor");
    auto stream = at::hip::getCurrentHIPStream();
    const float* fi = found_inf.has_value()
        ? found_inf->data_ptr<float>() : nullptr;
    for (size_t start = 0; start < tensors.size(); start += MT_MAX) {
        MTMeta m{};
        int chunks = 0, nt = 0;
        for (size_t i = start; i < std::min(tensors.size(), start + MT_MAX); ++i) {
            auto& g = tensors[i];
            TORCH_CHECK(g.is_cuda() && g.scalar_type() == at::kFloat &&
                        g.is_contiguous(), "scale expects contiguous fp32");
            m.b[nt] = g.data_ptr<float>();
            m.sizes[nt] = g.numel();
            m.chunk_start[nt] = chunks;
            chunks += ceil_div_i(g.numel(), MT_CHUNK);
            ++nt;
        }
        m.chunk_start[nt] = chunks;
        m.ntensors = nt;
        if (chunks == 0) continue;
        hipLaunchKernelGGL(k_mt_scale, dim3(chunks), dim3(MT_BLOCK), 0,
                           stream.stream(), m, coef.data_ptr<float>(), fi);
        HIP_CHECK_LAST();
    }
}

// -------------------------------------------------------------- fused SGD ---

// buf = mu*buf + g ; d = nesterov ? g + mu*buf : buf ; p -= lr*d
// With found_inf set, the step is a device-side no-op (amp overflow skip
// without a host sync).
// GS: lazy gradient clip — g is read as g * (*grad_scale), rounded once to
// fp32 before weight decay and the fmaf chain, i.e. bitwise what k_mt_scale
// followed by the GS=false kernel gives, without rewriting the gradients.
template <bool GS>
__global__ void k_mt_sgd(MTMeta m, float lr, float mu, float wd, float nesterov,
                         const float* __restrict__ found_inf,
                         const float* __restrict__ grad_scale) {
    if (found_inf && *found_inf != 0.0f) return;
    const float gs = GS ? *grad_scale : 1.0f;
    int t; long base, end;
    chunk_range(m, t, base, end);
    const float* __restrict__ g = m.a[t];
    float* __restrict__ p = m.b[t];
    float* __restrict__ buf = m.c[t];
    long vb = base >> 2, ve = end >> 2;
    for (long i = vb + threadIdx.x; i < ve; i += MT_BLOCK) {
        f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
        f32x4 bv = mu != 0.f ? reinterpret_cast<f32x4*>(buf)[i] : f32x4{};
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gi = gv[j];
            if (GS) gi = __fmul_rn(gi, gs);
            if (wd != 0.0f) gi = fmaf(wd, pv[j], gi);
            float d = gi;
            if (mu != 0.0f) {
                float b = fmaf(mu, bv[j], gi);
                bv[j] = b;
                d = (nesterov != 0.0f) ? fmaf(mu, b, gi) : b;
            }
            pv[j] = fmaf(-lr, d, pv[j]);
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
        if (mu != 0.f) reinterpret_cast<f32x4*>(buf)[i] = bv;
    }
    for (long i = ve * 4 + threadIdx.x; i < end; i += MT_BLOCK) {
        float gi = g[i];
        if (GS) gi = __fmul_rn(gi, gs);
        if (wd != 0.0f) gi = fmaf(wd, p[i], gi);
        float d = gi;
        if (mu != 0.0f) {
            float b = fmaf(mu, buf[i], gi);
            buf[i] = b;
            d = (nesterov != 0.0f) ? fmaf(mu, b, gi) : b;
        }
        p[i] = fmaf(-lr, d, p[i]);
    }
}

void fused_sgd(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
               std::vector<at::Tensor> bufs, double lr, double momentum,
               double wd, double nesterov,
               c10::optional<at::Tensor> found_inf,
               c10::optional<at::Tensor> grad_scale) {
    TORCH_CHECK(params.size() == grads.size());
    bool has_mu = momentum != 0.0;
    TORCH_CHECK(!has_mu || bufs.size() == params.size());
    auto stream = at::hip::getCurrentHIPStream();
    const float* fi = found_inf.has_value()
        ? found_inf->data_ptr<float>() : nullptr;
    const float* gs = nullptr;
    if (grad_scale.has_value()) {
        TORCH_CHECK(grad_scale->is_cuda() &&
                    grad_scale->scalar_type() == at::kFloat &&
                    grad_scale->numel() >= 1,
                    "fused_sgd: grad_scale must be a cuda fp32 tensor");
        gs = grad_scale->data_ptr<float>();
    }
    for (size_t start = 0; start < params.size(); start += MT_MAX) {
        MTMeta m{};
        int chunks = 0, nt = 0;
        for (size_t i = start; i < std::min(params.size(), start + MT_MAX); ++i) {
            m.a[nt] = grads[i].data_ptr<float>();
            m.b[nt] = params[i].data_ptr<float>();
            m.c[nt] = has_mu ? bufs[i].data_ptr<float>() : nullptr;
            m.sizes[nt] = params[i].numel();
            m.chunk_start[nt] = chunks;
            chunks += ceil_div_i(params[i].numel(), MT_CHUNK);
            ++nt;
        }
        m.chunk_start[nt] = chunks;
        m.ntensors = nt;
        if (chunks == 0) continue;
        if (gs)
            hipLaunchKernelGGL(k_mt_sgd<true>, dim3(chunks), dim3(MT_BLOCK), 0,
                               stream.stream(), m, (float)lr, (float)momentum,
                               (float)wd, (float)nesterov, fi, gs);
        else
            hipLaunchKernelGGL(k_mt_sgd<false>, dim3(chunks), dim3(MT_BLOCK),
                               0, stream.stream(), m, (float)lr,
                               (float)momentum, (float)wd, (float)nesterov,
                               fi, gs);
        HIP_CHECK_LAST();
    }
}

// -------------------------------------------------------------- fused LARS ---

// Layer-wise trust ratios (LARC "scale" formula) on the multi-tensor SGD
// path, three launches per MT_MAX group, each a device-side no-op when
// found_inf is set:
//   1. k_mt_lars_sqsum  per (tensor, chunk): sum p^2 and sum (g*gs)^2
//   2. k_mt_lars_ratio  per tensor: r = eta*|p| / (|g| + wd*|p| + eps)
//   3. k_mt_lars        k_mt_sgd's body with gi *= r before the momentum
// The ratio is a function of the partials alone (one block per tensor, a
// fixed summation order), so every block of a tensor steps with the same
// bits and the result does not depend on the grid.

// Same element->thread mapping and fmaf order as mt_chunk_pass<false, true>:
// with GS=false a chunk's g partial is bitwise k_mt_sqsum's.  GS squares
// __fmul_rn(g, gs), the value k_mt_scale would have left in memory, so the
// ratio is the same whether the clip was lazy or in place.
// partials[2*c] = sum p^2, partials[2*c+1] = sum g^2, c the global chunk.
template <bool GS>
__global__ void k_mt_lars_sqsum(MTMeta m, const float* __restrict__ found_inf,
                                const float* __restrict__ grad_scale,
                                float* __restrict__ partials, int chunk_base) {
    if (found_inf && *found_inf != 0.0f) return;
    const float gs = GS ? *grad_scale : 1.0f;
    int t; long base, end;
    chunk_range(m, t, base, end);
    const float* __restrict__ g = m.a[t];
    const float* __restrict__ p = m.b[t];
    float accp = 0.f, accg = 0.f;
    long vb = base >> 2, ve = end >> 2;
    for (long i = vb + threadIdx.x; i < ve; i += MT_BLOCK) {
        f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gj = gv[j];
            if (GS) gj = __fmul_rn(gj, gs);
            accg = fmaf(gj, gj, accg);
            accp = fmaf(pv[j], pv[j], accp);
        }
    }
    for (long i = ve * 4 + threadIdx.x; i < end; i += MT_BLOCK) {
        float gj = g[i];
        if (GS) gj = __fmul_rn(gj, gs);
        accg = fmaf(gj, gj, accg);
        accp = fmaf(p[i], p[i], accp);
    }
    float sp = mt_block_sum(accp);
    __syncthreads();  // mt_block_sum's LDS is reused by the second sum
    float sg = mt_block_sum(accg);
    if (threadIdx.x == 0) {
        long c = (long)chunk_base + blockIdx.x;
        partials[2 * c] = sp;
        partials[2 * c + 1] = sg;
    }
}

// One block per tensor.  Thread i sums the tensor's chunk partials i,
// i+MT_BLOCK, ... in double (a tensor may have thousands of chunks), then a
// fixed LDS tree; thread 0 forms the ratio in double and rounds it once.
// Zero-size tensors have no chunks: both norms are 0 and the ratio is 1.
__global__ void k_mt_lars_ratio(MTMeta m, const float* __restrict__ partials,
                                int chunk_base, float* __restrict__ ratios,
                                int tensor_base, double lr, double wd,
                                double eta, double eps, int trust_clip,
                                const float* __restrict__ found_inf) {
    if (found_inf && *found_inf != 0.0f) return;
    __shared__ double redp[MT_BLOCK];
    __shared__ double redg[MT_BLOCK];
    const int t = blockIdx.x;
    const int c0 = m.chunk_start[t], c1 = m.chunk_start[t + 1];
    double sp = 0.0, sg = 0.0;
    for (int c = c0 + threadIdx.x; c < c1; c += MT_BLOCK) {
        long k = 2 * ((long)chunk_base + c);
        sp += (double)partials[k];
        sg += (double)partials[k + 1];
    }
    redp[threadIdx.x] = sp;
    redg[threadIdx.x] = sg;
    __syncthreads();
    #pragma unroll
    for (int w = MT_BLOCK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            redp[threadIdx.x] += redp[threadIdx.x + w];
            redg[threadIdx.x] += redg[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double wn = sqrt(redp[0]), gn = sqrt(redg[0]);
    double r = 1.0;
    if (wn > 0.0 && gn > 0.0) {
        r = eta * wn / (gn + wd * wn + eps);
        if (trust_clip) r = fmin(r / lr, 1.0);
    }
    ratios[tensor_base + t] = (float)r;
}

// k_mt_sgd with the tensor's trust ratio applied to the decayed gradient:
// gi = (g*gs + wd*p) * r, rounded once, i.e. bitwise k_mt_scale(g, r)
// followed by k_mt_sgd when wd == 0.
template <bool GS>
__global__ void k_mt_lars(MTMeta m, float lr, float mu, float wd,
                          float nesterov, const float* __restrict__ found_inf,
                          const float* __restrict__ grad_scale,
                          const float* __restrict__ ratios, int tensor_base) {
    if (found_inf && *found_inf != 0.0f) return;
    const float gs = GS ? *grad_scale : 1.0f;
    int t; long base, end;
    chunk_range(m, t, base, end);
    const float r = ratios[tensor_base + t];
    const float* __restrict__ g = m.a[t];
    float* __restrict__ p = m.b[t];
    float* __restrict__ buf = m.c[t];
    long vb = base >> 2, ve = end >> 2;
    for (long i = vb + threadIdx.x; i < ve; i += MT_BLOCK) {
        f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
        f32x4 bv = mu != 0.f ? reinterpret_cast<f32x4*>(buf)[i] : f32x4{};
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gi = gv[j];
            if (GS) gi = __fmul_rn(gi, gs);
            if (wd != 0.0f) gi = fmaf(wd, pv[j], gi);
            gi = __fmul_rn(gi, r);
            float d = gi;
            if (mu != 0.0f) {
                float b = fmaf(mu, bv[j], gi);
                bv[j] = b;
                d = (nesterov != 0.0f) ? fmaf(mu, b, gi) : b;
            }
            pv[j] = fmaf(-lr, d, pv[j]);
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
        if (mu != 0.f) reinterpret_cast<f32x4*>(buf)[i] = bv;
    }
    for (long i = ve * 4 + threadIdx.x; i < end; i += MT_BLOCK) {
        float gi = g[i];
        if (GS) gi = __fmul_rn(gi, gs);
        if (wd != 0.0f) gi = fmaf(wd, p[i], gi);
        gi = __fmul_rn(gi, r);
        float d = gi;
        if (mu != 0.0f) {
            float b = fmaf(mu, buf[i], gi);
            buf[i] = b;
            d = (nesterov != 0.0f) ? fmaf(mu, b, gi) : b;
        }
        p[i] = fmaf(-lr, d, p[i]);
    }
}

// partials: 2 floats per (tensor, chunk); ratios: one float per tensor, in
// list order.  Both are indexed globally over the whole list, so the MT_MAX
// launch groups write disjoint ranges.
void fused_lars(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                std::vector<at::Tensor> bufs, at::Tensor partials,
                at::Tensor ratios, double lr, double momentum, double wd,
                double nesterov, double eta, double eps, bool trust_clip,
                c10::optional<at::Tensor> found_inf,
                c10::optional<at::Tensor> grad_scale) {
    TORCH_CHECK(params.size() == grads.size());
    bool has_mu = momentum != 0.0;
    TORCH_CHECK(!has_mu || bufs.size() == params.size());
    TORCH_CHECK(params.size() < (1UL << 30), "fused_lars: list too long");
    for (size_t i = 0; i < params.size(); ++i) {
        auto& p = params[i];
        auto& g = grads[i];
        TORCH_CHECK(p.is_cuda() && p.scalar_type() == at::kFloat &&
                    p.is_contiguous() && g.is_cuda() &&
                    g.scalar_type() == at::kFloat && g.is_contiguous() &&
                    g.numel() == p.numel(),
                    "fused_lars expects contiguous cuda fp32 params and "
                    "same-size grads");
        TORCH_CHECK(!has_mu || (bufs[i].is_cuda() &&
                                bufs[i].scalar_type() == at::kFloat &&
                                bufs[i].is_contiguous() &&
                                bufs[i].numel() == p.numel()),
                    "fused_lars: momentum buffer must match its parameter");
    }
    long total = mt_total_chunks(params);
    TORCH_CHECK(2 * total < (1L << 31), "multi-tensor list too large");
    TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == at::kFloat &&
                partials.is_contiguous() && partials.numel() >= 2 * total,
                "fused_lars: partials holds ", partials.numel(),
                " floats, need ", 2 * total, " (two per chunk)");
    TORCH_CHECK(ratios.is_cuda() && ratios.scalar_type() == at::kFloat &&
                ratios.is_contiguous() &&
                ratios.numel() >= (long)params.size(),
                "fused_lars: ratios holds ", ratios.numel(),
                " floats, need ", params.size(), " (one per tensor)");
    float* pp = partials.data_ptr<float>();
    float* rp = ratios.data_ptr<float>();
    auto stream = at::hip::getCurrentHIPStream();
    const float* fi = found_inf.has_value()
        ? found_inf->data_ptr<float>() : nullptr;
    const float* gs = nullptr;
    if (grad_scale.has_value()) {
        TORCH_CHECK(grad_scale->is_cuda() &&
                    grad_scale->scalar_type() == at::kFloat &&
                    grad_scale->numel() >= 1,
                    "fused_lars: grad_scale must be a cuda fp32 tensor");
        gs = grad_scale->data_ptr<float>();
    }
    int chunk_base = 0;
    for (size_t start = 0; start < params.size(); start += MT_MAX) {
        MTMeta m{};
        int chunks = 0, nt = 0;
        for (size_t i = start; i < std::min(params.size(), start + MT_MAX); ++i) {
            m.a[nt] = grads[i].data_ptr<float>();
            m.b[nt] = params[i].data_ptr<float>();
            m.c[nt] = has_mu ? bufs[i].data_ptr<float>() : nullptr;
            m.sizes[nt] = params[i].numel();
            m.chunk_start[nt] = chunks;
            chunks += ceil_div_i(params[i].numel(), MT_CHUNK);
            ++nt;
        }
        m.chunk_start[nt] = chunks;
        m.ntensors = nt;
        if (chunks > 0) {
            if (gs)
                hipLaunchKernelGGL(k_mt_lars_sqsum<true>, dim3(chunks),
                                   dim3(MT_BLOCK), 0, stream.stream(), m, fi,
                                   gs, pp, chunk_base);
            else
                hipLaunchKernelGGL(k_mt_lars_sqsum<false>, dim3(chunks),
                                   dim3(MT_BLOCK), 0, stream.stream(), m, fi,
                                   gs, pp, chunk_base);
            HIP_CHECK_LAST();
        }
        // also for a group of empty tensors: their ratios read 1
        hipLaunchKernelGGL(k_mt_lars_ratio, dim3(nt), dim3(MT_BLOCK), 0,
                           stream.stream(), m, pp, chunk_base, rp, (int)start,
                           lr, wd, eta, eps, trust_clip ? 1 : 0, fi);
        HIP_CHECK_LAST();
        if (chunks == 0) continue;
        if (gs)
            hipLaunchKernelGGL(k_mt_lars<true>, dim3(chunks), dim3(MT_BLOCK),
                               0, stream.stream(), m, (float)lr,
                               (float)momentum, (float)wd, (float)nesterov,
                               fi, gs, rp, (int)start);
        else
            hipLaunchKernelGGL(k_mt_lars<false>, dim3(chunks), dim3(MT_BLOCK),
                               0, stream.stream(), m, (float)lr,
                               (float)momentum, (float)wd, (float)nesterov,
                               fi, gs, rp, (int)start);
        HIP_CHECK_LAST();
        chunk_base += chunks;
    }
}

// ------------------------------------------------------ fused AdamW / LAMB ---

// Adam needs four arrays per tensor, one more than MTMeta holds.  A sibling
// struct (MTMeta and its kernels stay as they are); same (tensor, chunk)
// mapping, same MT_MAX / MT_CHUNK, global tensor and chunk indices.
struct MTMeta4 {
    const float* __restrict__ g[MT_MAX];
    float* __restrict__ p[MT_MAX];
    float* __restrict__ m[MT_MAX];
    float* __restrict__ v[MT_MAX];
    long sizes[MT_MAX];
    int chunk_start[MT_MAX + 1];
    int ntensors;
};

DEV_INLINE void chunk_range(const MTMeta4& m, int& t, long& base, long& end) {
    const int chunk = blockIdx.x;
    t = 0;
    while (t + 1 < m.ntensors && m.chunk_start[t + 1] <= chunk) ++t;
    long n = m.sizes[t];
    base = (long)(chunk - m.chunk_start[t]) * MT_CHUNK;
    end = base + MT_CHUNK < n ? base + MT_CHUNK : n;
}

// Per-tensor bias-correction coefficients of the current step, written by
// the tick and read by the step kernels: ADAM_NCOEF floats per tensor,
//   [0] lr / bc1      [1] sqrt(bc2)      [2] bc1      [3] bc2
// bc1 = 1 - beta1^step, bc2 = 1 - beta2^step.
constexpr int ADAM_NCOEF = 4;

// The step counter.  One thread per tensor of the launch group:
// steps[t] += 1 (fp32, exact below 2^24) and the coefficients of the new
// step, each computed in double and rounded to fp32 once.  It returns at
// once when found_inf is set, so a step that the amp overflow flag skips
// does not advance the bias correction.
__global__ void k_mt_adam_tick(float* __restrict__ steps,
                               float* __restrict__ coefs, int tensor_base,
                               int ntensors, double lr, double beta1,
                               double beta2,
                               const float* __restrict__ found_inf) {
    if (found_inf && *found_inf != 0.0f) return;
    const int t = threadIdx.x;
    if (t >= ntensors) return;
    const long k = (long)tensor_base + t;
    const float s = steps[k] + 1.0f;
    steps[k] = s;
    const double bc1 = 1.0 - pow(beta1, (double)s);
    const double bc2 = 1.0 - pow(beta2, (double)s);
    coefs[ADAM_NCOEF * k + 0] = (float)(lr / bc1);
    coefs[ADAM_NCOEF * k + 1] = (float)sqrt(bc2);
    coefs[ADAM_NCOEF * k + 2] = (float)bc1;
    coefs[ADAM_NCOEF * k + 3] = (float)bc2;
}

// Host-rounded constants of one step (each a double rounded to fp32 once).
struct AdamK {
    float b1, omb1;   // beta1, 1 - beta1
    float b2, omb2;   // beta2, 1 - beta2
    float eps;
    float wd;         // coupled (plain Adam) decay, and LAMB's wd
    float decay;      // 1 - lr*wd, the decoupled decay factor
    int decoupled;
};

// Moment update shared by AdamW and LAMB, one rounding per line:
//   t1 = omb1 * g            m = fma(b1, m, t1)
//   t2 = omb2 * g            t3 = t2 * g            v = fma(b2, v, t3)
DEV_INLINE void adam_moments(float g, float& m, float& v, const AdamK& k) {
    #pragma clang fp contract(off)
    m = fmaf(k.b1, m, __fmul_rn(k.omb1, g));
    v = fmaf(k.b2, v, __fmul_rn(__fmul_rn(k.omb2, g), g));
}

// The AdamW element update, exact fp32 operation order (one rounding each):
//   g  = g * gs                          (GS only)
//   g  = fma(wd, p, g)                   (plain Adam: !decoupled, wd != 0)
//   m, v                                 adam_moments
//   p  = p * decay                       (decoupled, wd != 0)
//   s  = sqrt(v)            q = s / c1         d = q + eps
//   r  = m / d              p = fma(-c0, r, p)
// c0 = lr/bc1, c1 = sqrt(bc2) from the tick.  sqrt and / are the correctly
// rounded ones (no fast-math in this build).
template <bool GS>
DEV_INLINE void adamw_elem(float g, float& p, float& m, float& v, float gs,
                           const AdamK& k, float c0, float c1) {
    #pragma clang fp contract(off)
    if (GS) g = __fmul_rn(g, gs);
    if (!k.decoupled && k.wd != 0.0f) g = fmaf(k.wd, p, g);
    adam_moments(g, m, v, k);
    if (k.decoupled && k.wd != 0.0f) p = __fmul_rn(p, k.decay);
    const float d = __fadd_rn(__fdiv_rn(sqrtf(v), c1), k.eps);
    p = fmaf(-c0, __fdiv_rn(m, d), p);
}

// One pass per (tensor, chunk): reads g, p, m, v, writes p, m, v; f32x4
// body and scalar tail as k_mt_sgd.  Device-side no-op under found_inf.
// GS reads the gradient as __fmul_rn(g, *grad_scale): bitwise k_mt_scale
// followed by the GS=false kernel.
template <bool GS>
__global__ void k_mt_adamw(MTMeta4 mt, AdamK k,
                           const float* __restrict__ coefs, int tensor_base,
                           const float* __restrict__ found_inf,
                           const float* __restrict__ grad_scale) {
    if (found_inf && *found_inf != 0.0f) return;
    const float gs = GS ? *grad_scale : 1.0f;
    int t; long base, end;
    chunk_range(mt, t, base, end);
    const float* __restrict__ cf = coefs + ADAM_NCOEF * ((long)tensor_base + t);
    const float c0 = cf[0], c1 = cf[1];
    const float* __restrict__ g = mt.g[t];
    float* __restrict__ p = mt.p[t];
    float* __restrict__ m = mt.m[t];
    float* __restrict__ v = mt.v[t];
    long vb = base >> 2, ve = end >> 2;
    for (long i = vb + threadIdx.x; i < ve; i += MT_BLOCK) {
        f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
        f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
        f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = pv[j], mj = mv[j], vj = vv[j];
            adamw_elem<GS>(gv[j], pj, mj, vj, gs, k, c0, c1);
            pv[j] = pj; mv[j] = mj; vv[j] = vj;
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
        reinterpret_cast<f32x4*>(m)[i] = mv;
        reinterpret_cast<f32x4*>(v)[i] = vv;
    }
    for (long i = ve * 4 + threadIdx.x; i < end; i += MT_BLOCK) {
        float pj = p[i], mj = m[i], vj = v[i];
        adamw_elem<GS>(g[i], pj, mj, vj, gs, k, c0, c1);
        p[i] = pj; m[i] = mj; v[i] = vj;
    }
}

// LAMB's update direction from the stored moments and the parameter, one
// rounding each:
//   mh = m / bc1      vh = v / bc2      s = sqrt(vh)      d = s + eps
//   q  = mh / d       u  = fma(wd, p, q)   (wd != 0; else u = q)
// Both the moments kernel (for |u|) and the step kernel call it on the same
// m, v, p, so no update buffer is needed.
DEV_INLINE float lamb_u(float p, float m, float v, float bc1, float bc2,
                        float eps, float wd) {
    #pragma clang fp contract(off)
    const float mh = __fdiv_rn(m, bc1);
    const float d = __fadd_rn(sqrtf(__fdiv_rn(v, bc2)), eps);
    const float q = __fdiv_rn(mh, d);
    return wd != 0.0f ? fmaf(wd, p, q) : q;
}

// LAMB launch 1: m and v in place (adam_moments on g*gs), then per-chunk
// sums of p^2 and u^2 in k_mt_lars_sqsum's layout: partials[2*c] = sum p^2,
// partials[2*c+1] = sum u^2, c the global chunk.  p is not written.
template <bool GS>
__global__ void k_mt_lamb_moments(MTMeta4 mt, AdamK k,
                                  const float* __restrict__ coefs,
                                  int tensor_base,
                                  const float* __restrict__ found_inf,
                                  const float* __restrict__ grad_scale,
                                  float* __restrict__ partials,
                                  int chunk_base) {
    if (found_inf && *found_inf != 0.0f) return;
    const float gs = GS ? *grad_scale : 1.0f;
    int t; long base, end;
    chunk_range(mt, t, base, end);
    const float* __restrict__ cf = coefs + ADAM_NCOEF * ((long)tensor_base + t);
    const float bc1 = cf[2], bc2 = cf[3];
    const float* __restrict__ g = mt.g[t];
    const float* __restrict__ p = mt.p[t];
    float* __restrict__ m = mt.m[t];
    float* __restrict__ v = mt.v[t];
    float accp = 0.f, accu = 0.f;
    long vb = base >> 2, ve = end >> 2;
    for (long i = vb + threadIdx.x; i < ve; i += MT_BLOCK) {
        f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
        f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
        f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gj = gv[j], mj = mv[j], vj = vv[j];
            if (GS) gj = __fmul_rn(gj, gs);
            adam_moments(gj, mj, vj, k);
            mv[j] = mj; vv[j] = vj;
            const float u = lamb_u(pv[j], mj, vj, bc1, bc2, k.eps, k.wd);
            accp = fmaf(pv[j], pv[j], accp);
            accu = fmaf(u, u, accu);
        }
        reinterpret_cast<f32x4*>(m)[i] = mv;
        reinterpret_cast<f32x4*>(v)[i] = vv;
    }
    for (long i = ve * 4 + threadIdx.x; i < end; i += MT_BLOCK) {
        float gj = g[i], mj = m[i], vj = v[i];
        if (GS) gj = __fmul_rn(gj, gs);
        adam_moments(gj, mj, vj, k);
        m[i] = mj; v[i] = vj;
        const float u = lamb_u(p[i], mj, vj, bc1, bc2, k.eps, k.wd);
        accp = fmaf(p[i], p[i], accp);
        accu = fmaf(u, u, accu);
    }
    float sp = mt_block_sum(accp);
    __syncthreads();  // mt_block_sum's LDS is reused by the second sum
    float su = mt_block_sum(accu);
    if (threadIdx.x == 0) {
        long c = (long)chunk_base + blockIdx.x;
        partials[2 * c] = sp;
        partials[2 * c + 1] = su;
    }
}

// LAMB launch 2: one block per tensor, the summation scheme of
// k_mt_lars_ratio.  r = |p| / |u| if both > 0 else 1, min(r, max_trust) with
// trust_clip; formed in double, rounded once.
__global__ void k_mt_lamb_ratio(MTMeta4 mt, const float* __restrict__ partials,
                                int chunk_base, float* __restrict__ ratios,
                                int tensor_base, int trust_clip,
                                double max_trust,
                                const float* __restrict__ found_inf) {
    if (found_inf && *found_inf != 0.0f) return;
    __shared__ double redp[MT_BLOCK];
    __shared__ double redu[MT_BLOCK];
    const int t = blockIdx.x;
    const int c0 = mt.chunk_start[t], c1 = mt.chunk_start[t + 1];
    double sp = 0.0, su = 0.0;
    for (int c = c0 + threadIdx.x; c < c1; c += MT_BLOCK) {
        long k = 2 * ((long)chunk_base + c);
        sp += (double)partials[k];
        su += (double)partials[k + 1];
    }
    redp[threadIdx.x] = sp;
    redu[threadIdx.x] = su;
    __syncthreads();
    #pragma unroll
    for (int w = MT_BLOCK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            redp[threadIdx.x] += redp[threadIdx.x + w];
            redu[threadIdx.x] += redu[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double wn = sqrt(redp[0]), un = sqrt(redu[0]);
    double r = 1.0;
    if (wn > 0.0 && un > 0.0) {
        r = wn / un;
        if (trust_clip) r = fmin(r, max_trust);
    }
    ratios[tensor_base + t] = (float)r;
}

// LAMB launch 3: u again from the stored m, v and the still-unchanged p
// (lamb_u, the same bits as launch 1 saw), then
//   a = lr * r (one rounding)      p = fma(-a, u, p)
__global__ void k_mt_lamb_step(MTMeta4 mt, float lr, float eps, float wd,
                               const float* __restrict__ coefs,
                               const float* __restrict__ ratios,
                               int tensor_base,
                               const float* __restrict__ found_inf) {
    if (found_inf && *found_inf != 0.0f) return;
    int t; long base, end;
    chunk_range(mt, t, base, end);
    const float* __restrict__ cf = coefs + ADAM_NCOEF * ((long)tensor_base + t);
    const float bc1 = cf[2], bc2 = cf[3];
    const float a = __fmul_rn(lr, ratios[tensor_base + t]);
    float* __restrict__ p = mt.p[t];
    const float* __restrict__ m = mt.m[t];
    const float* __restrict__ v = mt.v[t];
    long vb = base >> 2, ve = end >> 2;
    for (long i = vb + threadIdx.x; i < ve; i += MT_BLOCK) {
        f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
        f32x4 mv = reinterpret_cast<const f32x4*>(m)[i];
        f32x4 vv = reinterpret_cast<const f32x4*>(v)[i];
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float u = lamb_u(pv[j], mv[j], vv[j], bc1, bc2, eps, wd);
            pv[j] = fmaf(-a, u, pv[j]);
        }
        reinterpret_cast<f32x4*>(p)[i] = pv;
    }
    for (long i = ve * 4 + threadIdx.x; i < end; i += MT_BLOCK) {
        const float u = lamb_u(p[i], m[i], v[i], bc1, bc2, eps, wd);
        p[i] = fmaf(-a, u, p[i]);
    }
}

// Operand checks shared by fused_adamw and fused_lamb.  steps: one float
// per tensor, coefs: ADAM_NCOEF per tensor, both in list order.
static void adam_check(const char* who, const std::vector<at::Tensor>& params,
                       const std::vector<at::Tensor>& grads,
                       const std::vector<at::Tensor>& exp_avgs,
                       const std::vector<at::Tensor>& exp_avg_sqs,
                       const at::Tensor& steps, const at::Tensor& coefs,
                       const c10::optional<at::Tensor>& found_inf,
                       const c10::optional<at::Tensor>& grad_scale) {
    const size_t n = params.size();
    TORCH_CHECK(grads.size() == n && exp_avgs.size() == n &&
                exp_avg_sqs.size() == n, who, ": list lengths differ");
    TORCH_CHECK(n < (1UL << 28), who, ": list too long");
    auto ok = [](const at::Tensor& x, long numel) {
        return x.is_cuda() && x.scalar_type() == at::kFloat &&
               x.is_contiguous() && x.numel() == numel;
    };
    for (size_t i = 0; i < n; ++i) {
        const long ne = params[i].numel();
        TORCH_CHECK(ok(params[i], ne) && ok(grads[i], ne), who,
                    " expects contiguous cuda fp32 params and same-size "
                    "grads");
        TORCH_CHECK(ok(exp_avgs[i], ne) && ok(exp_avg_sqs[i], ne), who,
                    ": exp_avg / exp_avg_sq must match their parameter");
    }
    TORCH_CHECK(steps.is_cuda() && steps.scalar_type() == at::kFloat &&
                steps.is_contiguous() && steps.numel() >= (long)n,
                who, ": steps holds ", steps.numel(), " floats, need ", n,
                " (one per tensor)");
    TORCH_CHECK(coefs.is_cuda() && coefs.scalar_type() == at::kFloat &&
                coefs.is_contiguous() &&
                coefs.numel() >= (long)(ADAM_NCOEF * n),
                who, ": coefs holds ", coefs.numel(), " floats, need ",
                ADAM_NCOEF * n, " (", ADAM_NCOEF, " per tensor)");
    TORCH_CHECK(!found_inf.has_value() ||
                (found_inf->is_cuda() &&
                 found_inf->scalar_type() == at::kFloat &&
                 found_inf->numel() >= 1),
                who, ": found_inf must be a cuda fp32 tensor");
    TORCH_CHECK(!grad_scale.has_value() ||
                (grad_scale->is_cuda() &&
                 grad_scale->scalar_type() == at::kFloat &&
                 grad_scale->numel() >= 1),
                who, ": grad_scale must be a cuda fp32 tensor");
}

// Fills the kernarg struct for tensors [start, start + MT_MAX); returns the
// group's chunk count.
static int adam_pack(MTMeta4& m, size_t start,
                     const std::vector<at::Tensor>& params,
                     const std::vector<at::Tensor>& grads,
                     const std::vector<at::Tensor>& exp_avgs,
                     const std::vector<at::Tensor>& exp_avg_sqs) {
    int chunks = 0, nt = 0;
    for (size_t i = start; i < std::min(params.size(), start + MT_MAX); ++i) {
        m.g[nt] = grads[i].data_ptr<float>();
        m.p[nt] = params[i].data_ptr<float>();
        m.m[nt] = exp_avgs[i].data_ptr<float>();
        m.v[nt] = exp_avg_sqs[i].data_ptr<float>();
        m.sizes[nt] = params[i].numel();
        m.chunk_start[nt] = chunks;
        chunks += ceil_div_i(params[i].numel(), MT_CHUNK);
        ++nt;
    }
    m.chunk_start[nt] = chunks;
    m.ntensors = nt;
    return chunks;
}

static AdamK adam_consts(double lr, double beta1, double beta2, double eps,
                         double wd, bool decoupled) {
    AdamK k;
    k.b1 = (float)beta1;
    k.omb1 = (float)(1.0 - beta1);
    k.b2 = (float)beta2;
    k.omb2 = (float)(1.0 - beta2);
    k.eps = (float)eps;
    k.wd = (float)wd;
    k.decay = (float)(1.0 - lr * wd);
    k.decoupled = decoupled ? 1 : 0;
    return k;
}

// Tick + step per MT_MAX group.  No host sync, no H2D copy: everything the
// kernels need travels in the kernarg or is already on the device.
void fused_adamw(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                 std::vector<at::Tensor> exp_avgs,
                 std::vector<at::Tensor> exp_avg_sqs, at::Tensor steps,
                 at::Tensor coefs, double lr, double beta1, double beta2,
                 double eps, double wd, bool decoupled,
                 c10::optional<at::Tensor> found_inf,
                 c10::optional<at::Tensor> grad_scale) {
    adam_check("fused_adamw", params, grads, exp_avgs, exp_avg_sqs, steps,
               coefs, found_inf, grad_scale);
    mt_total_chunks(params);
    auto stream = at::hip::getCurrentHIPStream();
    const float* fi = found_inf.has_value()
        ? found_inf->data_ptr<float>() : nullptr;
    const float* gs = grad_scale.has_value()
        ? grad_scale->data_ptr<float>() : nullptr;
    float* sp = steps.data_ptr<float>();
    float* cp = coefs.data_ptr<float>();
    const AdamK k = adam_consts(lr, beta1, beta2, eps, wd, decoupled);
    for (size_t start = 0; start < params.size(); start += MT_MAX) {
        MTMeta4 m{};
        int chunks = adam_pack(m, start, params, grads, exp_avgs, exp_avg_sqs);
        hipLaunchKernelGGL(k_mt_adam_tick, dim3(1), dim3(MT_MAX), 0,
                           stream.stream(), sp, cp, (int)start, m.ntensors,
                           lr, beta1, beta2, fi);
        HIP_CHECK_LAST();
        if (chunks == 0) continue;
        if (gs)
            hipLaunchKernelGGL(k_mt_adamw<true>, dim3(chunks), dim3(MT_BLOCK),
                               0, stream.stream(), m, k, cp, (int)start, fi,
                               gs);
        else
            hipLaunchKernelGGL(k_mt_adamw<false>, dim3(chunks),
                               dim3(MT_BLOCK), 0, stream.stream(), m, k, cp,
                               (int)start, fi, gs);
        HIP_CHECK_LAST();
    }
}

// Tick + moments + ratio + step per MT_MAX group.  partials: 2 floats per
// (tensor, chunk); ratios: one float per tensor, list order; both indexed
// globally over the whole list.
void fused_lamb(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                std::vector<at::Tensor> exp_avgs,
                std::vector<at::Tensor> exp_avg_sqs, at::Tensor steps,
                at::Tensor coefs, at::Tensor partials, at::Tensor ratios,
                double lr, double beta1, double beta2, double eps, double wd,
                bool trust_clip, double max_trust,
                c10::optional<at::Tensor> found_inf,
                c10::optional<at::Tensor> grad_scale) {
    adam_check("fused_lamb", params, grads, exp_avgs, exp_avg_sqs, steps,
               coefs, found_inf, grad_scale);
    long total = mt_total_chunks(params);
    TORCH_CHECK(2 * total < (1L << 31), "multi-tensor list too large");
    TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == at::kFloat &&
                partials.is_contiguous() && partials.numel() >= 2 * total,
                "fused_lamb: partials holds ", partials.numel(),
                " floats, need ", 2 * total, " (two per chunk)");
    TORCH_CHECK(ratios.is_cuda() && ratios.scalar_type() == at::kFloat &&
                ratios.is_contiguous() &&
                ratios.numel() >= (long)params.size(),
                "fused_lamb: ratios holds ", ratios.numel(),
                " floats, need ", params.size(), " (one per tensor)");
    auto stream = at::hip::getCurrentHIPStream();
    const float* fi = found_inf.has_value()
        ? found_inf->data_ptr<float>() : nullptr;
    const float* gs = grad_scale.has_value()
        ? grad_scale->data_ptr<float>() : nullptr;
    float* sp = steps.data_ptr<float>();
    float* cp = coefs.data_ptr<float>();
    float* pp = partials.data_ptr<float>();
    float* rp = ratios.data_ptr<float>();
    const AdamK k = adam_consts(lr, beta1, beta2, eps, wd, true);
    int chunk_base = 0;
    for (size_t start = 0; start < params.size(); start += MT_MAX) {
        MTMeta4 m{};
        int chunks = adam_pack(m, start, params, grads, exp_avgs, exp_avg_sqs);
        hipLaunchKernelGGL(k_mt_adam_tick, dim3(1), dim3(MT_MAX), 0,
                           stream.stream(), sp, cp, (int)start, m.ntensors,
                           lr, beta1, beta2, fi);
        HIP_CHECK_LAST();
        if (chunks > 0) {
            if (gs)
                hipLaunchKernelGGL(k_mt_lamb_moments<true>, dim3(chunks),
                                   dim3(MT_BLOCK), 0, stream.stream(), m, k,
                                   cp, (int)start, fi, gs, pp, chunk_base);
            else
                hipLaunchKernelGGL(k_mt_lamb_moments<false>, dim3(chunks),
                                   dim3(MT_BLOCK), 0, stream.stream(), m, k,
                                   cp, (int)start, fi, gs, pp, chunk_base);
            HIP_CHECK_LAST();
        }
        // also for a group of empty tensors: their ratios read 1
        hipLaunchKernelGGL(k_mt_lamb_ratio, dim3(m.ntensors), dim3(MT_BLOCK),
                           0, stream.stream(), m, pp, chunk_base, rp,
                           (int)start, trust_clip ? 1 : 0, max_trust, fi);
        HIP_CHECK_LAST();
        if (chunks == 0) continue;
        hipLaunchKernelGGL(k_mt_lamb_step, dim3(chunks), dim3(MT_BLOCK), 0,
                           stream.stream(), m, (float)lr, k.eps, k.wd, cp, rp,
                           (int)start, fi);
        HIP_CHECK_LAST();
        chunk_base += chunks;
    }
}

long adam_ncoef() { return ADAM_NCOEF; }

// --------------------------------------------------------------- lookahead ---

// slow += alpha * (fast - slow); fast = slow     (reference lookahead.py:19-27)
__global__ void k_mt_lookahead(MTMeta m, float alpha,
                               const float* __restrict__ found_inf) {
    if (found_inf && *found_inf != 0.0f) return;
    int t; long base, end;
    chunk_range(m, t, base, end);
    float* __restrict__ fast = m.b[t];
    float* __restrict__ slow = m.c[t];
    long vb = base >> 2, ve = end >> 2;
    for (long i = vb + threadIdx.x; i < ve; i += MT_BLOCK) {
        f32x4 fv = reinterpret_cast<f32x4*>(fast)[i];
        f32x4 sv = reinterpret_cast<f32x4*>(slow)[i];
        #pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = fmaf(alpha, fv[j] - sv[j], sv[j]);
            sv[j] = s;
            fv[j] = s;
        }
        reinterpret_cast<f32x4*>(fast)[i] = fv;
        reinterpret_cast<f32x4*>(slow)[i] = sv;
    }
    for (long i = ve * 4 + threadIdx.x; i < end; i += MT_BLOCK) {
        float s = fmaf(alpha, fast[i] - slow[i], slow[i]);
        slow[i] = s;
        fast[i] = s;
    }
}

void fused_lookahead(std::vector<at::Tensor> fast, std::vector<at::Tensor> slow,
                     double alpha, c10::optional<at::Tensor> found_inf) {
    TORCH_CHECK(fast.size() == slow.size());
    auto stream = at::hip::getCurrentHIPStream();
    const float* fi = found_inf.has_value()
        ? found_inf->data_ptr<float>() : nullptr;
    for (size_t start = 0; start < fast.size(); start += MT_MAX) {
        MTMeta m{};
        int chunks = 0, nt = 0;
        for (size_t i = start; i < std::min(fast.size(), start + MT_MAX); ++i) {
            m.b[nt] = fast[i].data_ptr<float>();
            m.c[nt] = slow[i].data_ptr<float>();
            m.sizes[nt] = fast[i].numel();
            m.chunk_start[nt] = chunks;
            chunks += ceil_div_i(fast[i].numel(), MT_CHUNK);
            ++nt;
        }
        m.chunk_start[nt] = chunks;
        m.ntensors = nt;
        if (chunks == 0) continue;
        hipLaunchKernelGGL(k_mt_lookahead, dim3(chunks), dim3(MT_BLOCK), 0,
                           stream.stream(), m, (float)alpha, fi);
        HIP_CHECK_LAST();
    }
}

// ----------------------------------------------------------------- dropout ---

// Standalone counter-hash dropout (mask contract: common.h), for layers that
// are not a Linear+ReLU junction (those fuse it into the GEMM epilogue).
//   y[i] = round(x[i] * scale) where element i is kept, +0 where dropped,
// i the offset in the tensor's dense storage (contiguous or channels_last
// alike).  RELU applies relu first (the N <= 16 linear_act composition).
// The backward is the same map on dy: it REGENERATES the bits, because
// y == 0 says nothing about the mask here.  thr == 0 does no hashing.
// Eight elements and two hashes per thread; scalar tail, one hash each.
DEV_INLINE float drop_value(float v, bool relu, bool keep, float scale) {
    if (relu) v = v <= 0.f ? 0.f : v;      // NaN passes, -0 -> +0
    return keep ? __fmul_rn(v, scale) : 0.f;
}

template <bool RELU>
__global__ void k_dropout_bf16(const unsigned short* __restrict__ x,
                               unsigned short* __restrict__ y, long n,
                               unsigned thr, float scale,
                               unsigned long long seed, int aligned) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long stride = (long)gridDim.x * blockDim.x;
    long nv = aligned ? (n >> 3) : 0;
    for (long v = i; v < nv; v += stride) {
        s16x8 a = reinterpret_cast<const s16x8*>(x)[v];
        unsigned long long z0 = 0, z1 = 0;
        if (thr != 0) {
            z0 = drop_hash(seed, (unsigned long long)v * 2);
            z1 = drop_hash(seed, (unsigned long long)v * 2 + 1);
        }
        s16x8 o;
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
            bool keep = thr == 0 ||
                drop_lane(j < 4 ? z0 : z1, (unsigned)j) >= thr;
            o[j] = (short)f2us(drop_value(us2f((unsigned short)a[j]), RELU,
                                          keep, scale));
        }
        reinterpret_cast<s16x8*>(y)[v] = o;
    }
    for (long j = nv * 8 + i; j < n; j += stride) {
        bool keep = thr == 0 || drop_keep(seed, j, thr);
        y[j] = f2us(drop_value(us2f(x[j]), RELU, keep, scale));
    }
}

template <bool RELU>
__global__ void k_dropout_f32(const float* __restrict__ x,
                              float* __restrict__ y, long n, unsigned thr,
                              float scale, unsigned long long seed,
                              int aligned) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long stride = (long)gridDim.x * blockDim.x;
    long nv = aligned ? (n >> 3) : 0;
    for (long v = i; v < nv; v += stride) {
        #pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 a = reinterpret_cast<const f32x4*>(x)[v * 2 + h];
            unsigned long long z = 0;
            if (thr != 0) z = drop_hash(seed, (unsigned long long)v * 2 + h);
            #pragma unroll
            for (int j = 0; j < 4; ++j) {
                bool keep = thr == 0 || drop_lane(z, (unsigned)j) >= thr;
                a[j] = drop_value(a[j], RELU, keep, scale);
            }
            reinterpret_cast<f32x4*>(y)[v * 2 + h] = a;
        }
    }
    for (long j = nv * 8 + i; j < n; j += stride) {
        bool keep = thr == 0 || drop_keep(seed, j, thr);
        y[j] = drop_value(x[j], RELU, keep, scale);
    }
}

static at::Tensor launch_dropout(const at::Tensor& x, long thr, double scale,
                                 long call_seed, bool relu) {
    TORCH_CHECK(thr >= 0 && thr <= 65535, "dropout threshold ", thr,
                " outside [0, 65535]");
    TORCH_CHECK(thr != 0 || scale == 1.0, "thr == 0 needs scale == 1");
    TORCH_CHECK(x.is_cuda() && (x.scalar_type() == at::kBFloat16 ||
                                x.scalar_type() == at::kFloat),
                "dropout: cuda bf16 or fp32 expected");
    // dense storage, indexed in storage order
    TORCH_CHECK(x.is_contiguous() ||
                (x.dim() == 4 &&
                 x.is_contiguous(at::MemoryFormat::ChannelsLast)),
                "dropout: contiguous or channels_last tensor expected");
    auto y = at::empty_like(x);     // keeps x's strides
    long n = x.numel();
    if (n == 0) return y;
    int aligned = (((uintptr_t)x.data_ptr() | (uintptr_t)y.data_ptr()) & 15)
                  == 0;
    int blocks = (int)std::min<long>(4096, ceil_div_i(ceil_div_i(n, 8), 256));
    auto stream = at::hip::getCurrentHIPStream();
    unsigned long long seed = (unsigned long long)call_seed;
    if (x.scalar_type() == at::kBFloat16) {
        auto xp = reinterpret_cast<const unsigned short*>(x.data_ptr());
        auto yp = reinterpret_cast<unsigned short*>(y.data_ptr());
        if (relu)
            hipLaunchKernelGGL(k_dropout_bf16<true>, dim3(blocks), dim3(256),
                               0, stream.stream(), xp, yp, n, (unsigned)thr,
                               (float)scale, seed, aligned);
        else
            hipLaunchKernelGGL(k_dropout_bf16<false>, dim3(blocks), dim3(256),
                               0, stream.stream(), xp, yp, n, (unsigned)thr,
                               (float)scale, seed, aligned);
    } else {
        if (relu)
            hipLaunchKernelGGL(k_dropout_f32<true>, dim3(blocks), dim3(256),
                               0, stream.stream(), x.data_ptr<float>(),
                               y.data_ptr<float>(), n, (unsigned)thr,
                               (float)scale, seed, aligned);
        else
            hipLaunchKernelGGL(k_dropout_f32<false>, dim3(blocks), dim3(256),
                               0, stream.stream(), x.data_ptr<float>(),
                               y.data_ptr<float>(), n, (unsigned)thr,
                               (float)scale, seed, aligned);
    }
    HIP_CHECK_LAST();
    return y;
}

at::Tensor dropout_fwd(at::Tensor x, long thr, double scale, long call_seed) {
    return launch_dropout(x, thr, scale, call_seed, false);
}

at::Tensor dropout_bwd(at::Tensor dy, long thr, double scale,
                       long call_seed) {
    return launch_dropout(dy, thr, scale, call_seed, false);
}

at::Tensor relu_dropout_fwd(at::Tensor x, long thr, double scale,
                            long call_seed) {
    return launch_dropout(x, thr, scale, call_seed, true);
}

// ------------------------------------------------------------------- casts ---

__global__ void k_f32_to_bf16(const float* __restrict__ in,
                              unsigned short* __restrict__ out, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long stride = (long)gridDim.x * blockDim.x;
    long nv = n >> 2;
    for (long v = i; v < nv; v += stride) {
        f32x4 f = reinterpret_cast<const f32x4*>(in)[v];
        s16x4 o;
        o[0] = f2us(f[0]); o[1] = f2us(f[1]); o[2] = f2us(f[2]); o[3] = f2us(f[3]);
        reinterpret_cast<s16x4*>(out)[v] = o;
    }
    for (long j = nv * 4 + i; j < n; j += stride)
        out[j] = f2us(in[j]);
}

at::Tensor cast_to_bf16(at::Tensor x) {
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.is_contiguous());
    auto y = at::empty_like(x, x.options().dtype(at::kBFloat16));
    long n = x.numel();
    int blocks = (int)std::min<long>(2048, (n / 4 + 255) / 256 + 1);
    auto stream = at::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(k_f32_to_bf16, dim3(blocks), dim3(256), 0, stream.stream(),
                       x.data_ptr<float>(),
                       reinterpret_cast<unsigned short*>(y.data_ptr()), n);
    HIP_CHECK_LAST();
    return y;
}

// ------------------------------------------------- conv weight packing ---

// One pass over the fp32 master weight [K,C,R,S] producing BOTH bf16
// operand layouts: nhwc [K,R,S,Cp] (forward) and wt2 [Cp, R*S*K] (dgrad),
// with optional zero-padding of C to Cp=8 (the C<8 stem path).  Replaces
// the per-step chain of to(bf16) + contiguous(channels_last) + permute +
// reshape + contiguous ATen launches (SURVEY N4's cast layer).
__global__ void k_pack_conv_weight(const float* __restrict__ w,
                                   bf16* __restrict__ nhwc,
                                   bf16* __restrict__ wt2,
                                   int K, int C, int RS, int Cp) {
    long total = (long)K * Cp * RS;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long stride = (long)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        int c = i % Cp;
        long r2 = i / Cp;
        int rs = r2 % RS;
        int k = r2 / RS;
        float v = c < C ? w[((long)k * C + c) * RS + rs] : 0.f;
        bf16 b = f2bf(v);
        nhwc[((long)k * RS + rs) * Cp + c] = b;           // [K,R,S,Cp]
        if (wt2)
            wt2[((long)c * RS + rs) * K + k] = b;         // [Cp, RS*K]
    }
}

std::vector<at::Tensor> pack_conv_weight(at::Tensor w, bool pad8,
                                         bool want_wt2) {
    TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kFloat &&
                w.is_contiguous());
    int K = w.size(0), C = w.size(1), R = w.size(2), S = w.size(3);
    int Cp = pad8 ? 8 : C;
    int RS = R * S;
    auto opts = w.options().dtype(at::kBFloat16);
    // nhwc tensor carries channels_last metadata for [K,Cp,R,S]
    auto nhwc = at::empty({K, Cp, R, S},
                          opts.memory_format(at::MemoryFormat::ChannelsLast));
    at::Tensor wt2;
    bf16* wt2p = nullptr;
    if (want_wt2) {
        wt2 = at::empty({Cp, (long)RS * K}, opts);
        wt2p = reinterpret_cast<bf16*>(wt2.data_ptr());
    }
    long total = (long)K * Cp * RS;
    auto stream = at::hip::getCurrentHIPStream();
    int blocks = std::min<long>(2048, ceil_div_i(total, 256));
    hipLaunchKernelGGL(k_pack_conv_weight, dim3(blocks), dim3(256), 0,
                       stream.stream(), w.data_ptr<float>(),
                       reinterpret_cast<bf16*>(nhwc.data_ptr()), wt2p,
                       K, C, RS, Cp);
    HIP_CHECK_LAST();
    if (want_wt2) return {nhwc, wt2};
    return {nhwc};
}

// Zero-pad channels to 8 in ONE pass (replaces at::zeros + slice copy_ —
// two ATen launches per step on the C<8 stem path).
__global__ void k_pad8(const bf16* __restrict__ x, bf16* __restrict__ xp,
                       long total_px, int C) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long stride = (long)gridDim.x * blockDim.x;
    for (; i < total_px; i += stride) {
        s16x8 o = {};
        const bf16* src = x + i * C;
        for (int c = 0; c < C; ++c) o[c] = *(const short*)&src[c];
        reinterpret_cast<s16x8*>(xp)[i] = o;
    }
}

at::Tensor pad8_channels(at::Tensor x) {
    // x: [N,C<8,H,W] channels_last bf16 -> [N,8,H,W] channels_last
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16);
    int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
    TORCH_CHECK(C < 8);
    auto xp = at::empty({N, 8, H, W},
                        x.options().memory_format(at::MemoryFormat::ChannelsLast));
    long total = (long)N * H * W;
    auto stream = at::hip::getCurrentHIPStream();
    int blocks = std::min<long>(4096, ceil_div_i(total, 256));
    hipLaunchKernelGGL(k_pad8, dim3(blocks), dim3(256), 0, stream.stream(),
                       reinterpret_cast<const bf16*>(x.data_ptr()),
                       reinterpret_cast<bf16*>(xp.data_ptr()), total, C);
    HIP_CHECK_LAST();
    return xp;
}

// NHWC flatten boundary (Toy_Net conv->dense junction): [N,C,H,W]
// channels_last bf16 -> [N, C*H*W] in NCHW semantic order (the order the
// reference's fc1 weight layout expects; reference utils/model.py:23-25),
// plus the inverse for backward.  Replaces two ~23 us strided ATen
// permute-copies per step: here the fwd gather is coalesced across the
// c-threads (consecutive c -> consecutive addresses within each s row)
// and each thread writes its HW-contiguous chunk with s16x8 stores.
__global__ void k_nhwc_flatten(const bf16* __restrict__ x,
                               bf16* __restrict__ y, int C, int HW) {
    const int c = blockIdx.y * blockDim.x + threadIdx.x;
    const long b = blockIdx.x;
    if (c >= C) return;
    const bf16* src = x + (long)b * HW * C + c;
    bf16* dst = y + ((long)b * C + c) * HW;
    // NO runtime-indexed staging array (it would spill to scratch — the
    // HW bound is runtime); fixed-8 inner unroll keeps the gather in
    // registers and the store a single s16x8.
    if ((HW & 7) == 0) {
        for (int s8 = 0; s8 < HW; s8 += 8) {
            s16x8 v;
            #pragma unroll
            for (int k = 0; k < 8; ++k)
                v[k] = *(const short*)&src[(long)(s8 + k) * C];
            *reinterpret_cast<s16x8*>(&dst[s8]) = v;
        }
    } else {
        for (int s = 0; s < HW; ++s)
            *(short*)&dst[s] = *(const short*)&src[(long)s * C];
    }
}

__global__ void k_nhwc_unflatten(const bf16* __restrict__ dy,
                                 bf16* __restrict__ dx, int C, int HW) {
    const int c = blockIdx.y * blockDim.x + threadIdx.x;
    const long b = blockIdx.x;
    if (c >= C) return;
    const bf16* src = dy + ((long)b * C + c) * HW;   // contiguous chunk
    bf16* dst = dx + (long)b * HW * C + c;
    if ((HW & 7) == 0) {
        for (int s8 = 0; s8 < HW; s8 += 8) {
            const s16x8 v = *reinterpret_cast<const s16x8*>(&src[s8]);
            #pragma unroll
            for (int k = 0; k < 8; ++k)
                *(short*)&dst[(long)(s8 + k) * C] = v[k];
        }
    } else {
        for (int s = 0; s < HW; ++s)
            *(short*)&dst[(long)s * C] = *(const short*)&src[s];
    }
}

at::Tensor nhwc_flatten(at::Tensor x) {
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 &&
                x.dim() == 4, "nhwc_flatten: 4D cuda bf16 expected");
    TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
                "nhwc_flatten: channels_last expected");
    const int N = x.size(0), C = x.size(1);
    const int HW = x.size(2) * x.size(3);
    TORCH_CHECK(HW <= 64, "nhwc_flatten: HW too large");
    auto y = at::empty({(long)N, (long)C * HW}, x.options());
    auto stream = at::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(k_nhwc_flatten,
                       dim3(N, ceil_div_i(C, 256)), dim3(256), 0,
                       stream.stream(),
                       reinterpret_cast<const bf16*>(x.data_ptr()),
                       reinterpret_cast<bf16*>(y.data_ptr()), C, HW);
    HIP_CHECK_LAST();
    return y;
}

at::Tensor nhwc_unflatten(at::Tensor dy, long C, long H, long W) {
    TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16 &&
                dy.dim() == 2 && dy.is_contiguous(),
                "nhwc_unflatten: 2D contiguous cuda bf16 expected");
    const long N = dy.size(0);
    const int HW = (int)(H * W);
    TORCH_CHECK(dy.size(1) == C * HW && HW <= 64);
    auto dx = at::empty({N, C, H, W},
                        dy.options().memory_format(at::MemoryFormat::ChannelsLast));
    auto stream = at::hip::getCurrentHIPStream();
    hipLaunchKernelGGL(k_nhwc_unflatten,
                       dim3(N, ceil_div_i((int)C, 256)), dim3(256), 0,
                       stream.stream(),
                       reinterpret_cast<const bf16*>(dy.data_ptr()),
                       reinterpret_cast<bf16*>(dx.data_ptr()), (int)C, HW);
    HIP_CHECK_LAST();
    return dx;
}
