// dllama_amd — Q80 quantize, rmsnorm variants, embedding, argmax and elementwise kernels.

#include "dllama_common.h"

// ------------------------------------------------------------------ q80 quantize
// f32 [rows, n] -> int8 q [rows, n], f32 scale [rows, n/32], f32 bsum [rows, n/32]
// (role of reference quantizeF32toQ80, nn-quants.cpp:67 and the
//  cast-forward-f32-q80 Vulkan shader). bsum = sum of the int8 values,
// used by the GEMV to fold the Q40 nibble offset.
__global__ void k_q80_quantize(const float *__restrict__ x,
                               int8_t *__restrict__ q,
                               float *__restrict__ s,
                               float *__restrict__ bs,
                               int n_blocks_total) {
    // one 32-lane group per block
    int gid = (blockIdx.x * blockDim.x + threadIdx.x) / 32;
    int lane = threadIdx.x & 31;
    if (gid >= n_blocks_total) return;
    const Q80Lane c = q80_quant_group32(x[gid * QB + lane]);
    q[gid * QB + lane] = (int8_t)c.qf;
    const float bsum = group32_reduce_sum(c.qf);
    if (lane == 0) {
        s[gid] = c.d;
        bs[gid] = bsum;
    }
}

// ------------------------------------------------------------------ rmsnorm
// y = x * w / sqrt(mean(x^2)+eps) (reference invRms_F32 + rmsNorm_F32,
// nn-cpu-ops.cpp:114-175, fused). One workgroup per row.
__global__ void k_rmsnorm(const float *__restrict__ x,
                          const float *__restrict__ w,
                          float *__restrict__ y,
                          int n, float eps) {
    const float *row = x + (int64_t)blockIdx.x * n;
    float *out = y + (int64_t)blockIdx.x * n;
    float acc = 0.0f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        float v = row[i];
        acc += v * v;
    }
    __shared__ float red[16];
    acc = wave_reduce_sum(acc);
    int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (lane == 0) red[wid] = acc;
    __syncthreads();
    int nw = blockDim.x / WAVE;
    float total = 0.0f;
    for (int i = 0; i < nw; i++) total += red[i];
    float inv = rsqrtf(total / n + eps);
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        out[i] = row[i] * inv * w[i];
}

// fused rmsnorm + q80 quantize: avoids a full extra activation pass
// (reference runs inv_rms -> rms_norm -> cast as three ops).
__global__ void k_rmsnorm_q80(const float *__restrict__ x,
                              const float *__restrict__ w,
                              int8_t *__restrict__ q,
                              float *__restrict__ s,
                              float *__restrict__ bs,
                              int n, float eps) {
    const float *row = x + (int64_t)blockIdx.x * n;
    float acc = 0.0f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        float v = row[i];
        acc += v * v;
    }
    __shared__ float red[16];
    acc = wave_reduce_sum(acc);
    int wid = threadIdx.x / WAVE, lane64 = threadIdx.x % WAVE;
    if (lane64 == 0) red[wid] = acc;
    __syncthreads();
    int nw = blockDim.x / WAVE;
    float total = 0.0f;
    for (int i = 0; i < nw; i++) total += red[i];
    float inv = rsqrtf(total / n + eps);

    int nb = n / QB;
    int8_t *qrow = q + (int64_t)blockIdx.x * n;
    float *srow = s + (int64_t)blockIdx.x * nb;
    float *bsrow = bs + (int64_t)blockIdx.x * nb;
    int lane32 = threadIdx.x & 31;
    for (int blk = threadIdx.x / 32; blk < nb; blk += blockDim.x / 32) {
        const Q80Lane c = q80_quant_group32(
            row[blk * QB + lane32] * inv * w[blk * QB + lane32]);
        qrow[blk * QB + lane32] = (int8_t)c.qf;
        const float bsum = group32_reduce_sum(c.qf);
        if (lane32 == 0) { srow[blk] = c.d; bsrow[blk] = bsum; }
    }
}

// per-head rmsnorm (Qwen3 q/k-norm; reference multi-column OP_INV_RMS +
// OP_RMS_NORM, llm.cpp:178-187). x [rows, hd], w [hd]; hd <= 512.
__global__ void k_rmsnorm_rows(const float *__restrict__ x,
                               const float *__restrict__ w,
                               float *__restrict__ y,
                               int hd, float eps) {
    const float *row = x + (int64_t)blockIdx.x * hd;
    float *out = y + (int64_t)blockIdx.x * hd;
    float acc = 0.0f;
    for (int i = threadIdx.x; i < hd; i += blockDim.x) {
        float v = row[i];
        acc += v * v;
    }
    acc = wave_reduce_sum(acc);  // blockDim == 64 (one wave)
    float inv = rsqrtf(acc / hd + eps);
    for (int i = threadIdx.x; i < hd; i += blockDim.x)
        out[i] = row[i] * inv * w[i];
}

// per-head rmsnorm on a slice of the fused QKV buffer (Qwen3 q/k-norm on
// strided rows): batch b, head h -> row at buf + b*ld + off + h*hd.
__global__ void k_rmsnorm_rows_s(float *__restrict__ buf, int ld, int off,
                                 int heads, const float *__restrict__ w,
                                 int hd, float eps) {
    const int b = blockIdx.x / heads;
    const int h = blockIdx.x % heads;
    float *row = buf + (int64_t)b * ld + off + h * hd;
    float acc = 0.0f;
    for (int i = threadIdx.x; i < hd; i += blockDim.x) {
        const float v = row[i];
        acc += v * v;
    }
    acc = wave_reduce_sum(acc);  // blockDim == 64
    const float inv = rsqrtf(acc / hd + eps);
    for (int i = threadIdx.x; i < hd; i += blockDim.x)
        row[i] = row[i] * inv * w[i];
}

// ---------------------------------------------- fused residual+rmsnorm(+q80)
// x[row] += partial[row] (ADD), then rmsnorm with w; output either f32 y
// (!QUANT) or the Q80 triple (QUANT). Fuses the reference's
// merge_add -> inv_rms -> rms_norm -> cast chain (llm.cpp:263-270) into one
// kernel: one extra pass saved per layer half, and the B=1 row gets a full
// 1024-thread workgroup with float4 traffic.
template <bool ADD, bool QUANT>
__global__ void k_add_rmsnorm(float *__restrict__ x,
                              const float *__restrict__ partial,
                              const float *__restrict__ w,
                              float *__restrict__ y,
                              int8_t *__restrict__ q,
                              float *__restrict__ s,
                              float *__restrict__ bs,
                              int n, float eps) {
    extern __shared__ float lds[];  // n floats: x staged once, re-read from LDS
    const int64_t base = (int64_t)blockIdx.x * n;
    float acc = 0.0f;
    for (int i = threadIdx.x * 4; i < n; i += blockDim.x * 4) {
        float4 v = *reinterpret_cast<const float4 *>(x + base + i);
        if (ADD) {
            const float4 p = *reinterpret_cast<const float4 *>(partial + base + i);
            v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
            *reinterpret_cast<float4 *>(x + base + i) = v;
        }
        *reinterpret_cast<float4 *>(lds + i) = v;
        acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    __shared__ float red[16];
    acc = wave_reduce_sum(acc);
    const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (lane == 0) red[wid] = acc;
    __syncthreads();
    const int nw = blockDim.x / WAVE;
    float total = 0.0f;
    for (int i = 0; i < nw; i++) total += red[i];
    const float inv = rsqrtf(total / n + eps);

    if (!QUANT) {
        for (int i = threadIdx.x * 4; i < n; i += blockDim.x * 4) {
            const float4 v = *reinterpret_cast<const float4 *>(lds + i);
            const float4 wv = *reinterpret_cast<const float4 *>(w + i);
            float4 o;
            o.x = v.x * inv * wv.x; o.y = v.y * inv * wv.y;
            o.z = v.z * inv * wv.z; o.w = v.w * inv * wv.w;
            *reinterpret_cast<float4 *>(y + base + i) = o;
        }
    } else {
        const int nb = n / QB;
        const int lane32 = threadIdx.x & 31;
        for (int blk = threadIdx.x / 32; blk < nb; blk += blockDim.x / 32) {
            const int i = blk * QB + lane32;
            const Q80Lane c = q80_quant_group32(lds[i] * inv * w[i]);
            q[base + i] = (int8_t)c.qf;
            const float bsum = group32_reduce_sum(c.qf);
            if (lane32 == 0) {
                s[(int64_t)blockIdx.x * nb + blk] = c.d;
                bs[(int64_t)blockIdx.x * nb + blk] = bsum;
            }
        }
    }
}

// embedding row gather (replaces torch index_select inside the decode graph
// — the ATen gather kernel costs ~40 us/step there; reference OP_EMBEDDING,
// nn-cpu-ops.cpp:982-1008).
__global__ void k_embed_gather(const float *__restrict__ table,
                               const long *__restrict__ tokens,
                               float *__restrict__ x, int dim,
                               float *__restrict__ ssq) {
    const int b = blockIdx.y;
    const int64_t src = (int64_t)tokens[b] * dim;
    float local = 0.0f;
    for (int i = (blockIdx.x * blockDim.x + threadIdx.x) * 4; i < dim;
         i += gridDim.x * blockDim.x * 4) {
        const float4 v = *reinterpret_cast<const float4 *>(table + src + i);
        *reinterpret_cast<float4 *>(x + (int64_t)b * dim + i) = v;
        local += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    if (ssq != nullptr) ssq_block_add<0>(ssq, b, local);
}

// ------------------------------------------- wide norm from precomputed ssq
// The residual row's sum-of-squares arrives precomputed (GEMV RESID epilogue
// / embed / merge-add), so the rmsnorm becomes one wide pass with no
// in-kernel reduction: quantized (Q80 triple) or f32 output.
__global__ void k_norm_quant(const float *__restrict__ x,
                             const float *__restrict__ w,
                             const float *__restrict__ ssq,
                             int8_t *__restrict__ q,
                             float *__restrict__ s,
                             float *__restrict__ bs,
                             float *__restrict__ yout,
                             int n, float eps, int deferred) {
    const int b = blockIdx.y;
    // deferred: emit x*w with the inv_rms factored out of the scale — the
    // consuming GEMV applies inv from ssq (PRO==2); codes are identical
    // either way (q depends only on intra-block ratios)
    const float inv = deferred ? 1.0f : rsqrtf(ssq_total(ssq, b) / n + eps);
    const int nb = n / QB;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int blk = gid / 32;
    const int lane = threadIdx.x & 31;
    if (blk >= nb) return;
    const int i = blk * QB + lane;
    const float v = x[(int64_t)b * n + i] * inv * w[i];
    if (yout != nullptr) yout[(int64_t)b * n + i] = v;
    const Q80Lane c = q80_quant_group32(v);
    q[(int64_t)b * n + i] = (int8_t)c.qf;
    const float bsum = group32_reduce_sum(c.qf);
    if (lane == 0) {
        s[(int64_t)b * nb + blk] = c.d;
        bs[(int64_t)b * nb + blk] = bsum;
    }
}

__global__ void k_norm_f32(const float *__restrict__ x,
                           const float *__restrict__ w,
                           const float *__restrict__ ssq,
                           float *__restrict__ y,
                           int n, float eps) {
    const int b = blockIdx.y;
    const float inv = rsqrtf(ssq_total(ssq, b) / n + eps);
    for (int i = (blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n;
         i += gridDim.x * blockDim.x * 4) {
        const float4 v = *reinterpret_cast<const float4 *>(x + (int64_t)b * n + i);
        const float4 wv = *reinterpret_cast<const float4 *>(w + i);
        float4 o;
        o.x = v.x * inv * wv.x; o.y = v.y * inv * wv.y;
        o.z = v.z * inv * wv.z; o.w = v.w * inv * wv.w;
        *reinterpret_cast<float4 *>(y + (int64_t)b * n + i) = o;
    }
}

// x[b] += p[b] with per-row sum-of-squares accumulation (residual fold for
// paths that produce a separate partial: MoE weighted sum, f32 TP sync).
__global__ void k_add_ssq(float *__restrict__ x,
                          const float *__restrict__ p,
                          float *__restrict__ ssq, int n) {
    const int b = blockIdx.y;
    float local = 0.0f;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gridDim.x * blockDim.x) {
        const float v = x[(int64_t)b * n + i] + p[(int64_t)b * n + i];
        x[(int64_t)b * n + i] = v;
        local += v * v;
    }
    ssq_block_add<0>(ssq, b, local);
}

// stage 2 of the on-device greedy argmax: reduce the per-workgroup bests the
// logits GEMV wrote to scratch (no atomics anywhere — a single-slot atomicMax
// across 32k workgroups serializes on one cacheline and costs >1 ms).
__global__ void k_token_from_argmax(long *__restrict__ token,
                                    const unsigned long long *__restrict__ scratch,
                                    int count) {
    unsigned long long best = 0ull;
    for (int i = threadIdx.x; i < count; i += blockDim.x)
        best = max(best, scratch[i]);
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        best = max(best, (unsigned long long)__shfl_xor((long long)best, off, WAVE));
    __shared__ unsigned long long red[16];
    const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (lane == 0) red[wid] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < blockDim.x / WAVE; i++) best = max(best, red[i]);
        best = max(best, red[0]);
        token[0] = (long)(0x7FFFFFFF - (int)(best & 0xFFFFFFFFu));
    }
}

// generic argmax stage 1 over a flat f32 array (the TP greedy path: argmax
// of the gathered full logits). Each block writes its packed best to
// scratch[blockIdx]; k_token_from_argmax reduces scratch.
__global__ void k_argmax_stage1(const float *__restrict__ x, int64_t n,
                                unsigned long long *__restrict__ scratch) {
    unsigned long long best = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        best = max(best, argmax_pack(x[i], (int)i));
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        best = max(best, (unsigned long long)__shfl_xor((long long)best, off, WAVE));
    __shared__ unsigned long long red[16];
    const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (lane == 0) red[wid] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < blockDim.x / WAVE; i++) best = max(best, red[i]);
        scratch[blockIdx.x] = best;
    }
}

// ------------------------------------------------------------------ swiglu (+q80)
// d = silu(a) * g, quantized straight to Q80 (reference OP_SILU + OP_MUL +
// OP_CAST fused; silu nn-cpu-ops.cpp:462-500).
template <bool GELU>
__global__ void k_swiglu_q80(const float *__restrict__ a,
                             const float *__restrict__ g,
                             int lda, int n,
                             int8_t *__restrict__ q,
                             float *__restrict__ s,
                             float *__restrict__ bs,
                             int n_blocks_total) {
    int gid = (blockIdx.x * blockDim.x + threadIdx.x) / 32;
    int lane = threadIdx.x & 31;
    if (gid >= n_blocks_total) return;
    const int nb = n / QB;
    const int r = gid / nb;
    const int i = (gid % nb) * QB + lane;
    float av = a[(int64_t)r * lda + i];
    float gv = g[(int64_t)r * lda + i];
    // silu (reference nn-cpu-ops.cpp:462) or tanh-approx gelu (:454)
    float act = GELU
        ? 0.5f * av * (1.0f + tanhf(0.797884560802865f * (av + 0.044715f * av * av * av)))
        : av / (1.0f + __expf(-av));
    const Q80Lane c = q80_quant_group32(act * gv);
    q[gid * QB + lane] = (int8_t)c.qf;
    const float bsum = group32_reduce_sum(c.qf);
    if (lane == 0) { s[gid] = c.d; bs[gid] = bsum; }
}

__global__ void k_silu_mul(const float *__restrict__ a,
                           const float *__restrict__ g,
                           float *__restrict__ out,
                           int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        float av = a[i];
        out[i] = av / (1.0f + __expf(-av)) * g[i];
    }
}

// x += y (residual merge for the f32/TP=1 path)
__global__ void k_add(float *__restrict__ x, const float *__restrict__ y, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        x[i] += y[i];
}

__global__ void k_inc(int *__restrict__ pos, int delta) {
    if (threadIdx.x == 0 && blockIdx.x == 0) pos[0] += delta;
}

// ============================================================== host bindings

void q80_quantize(torch::Tensor x, torch::Tensor q, torch::Tensor s, torch::Tensor bs) {
    CHECK_CUDA(x); CHECK_CONT(x);
    const int64_t blocks = x.numel() / QB;
    const int threads = 256;
    hipLaunchKernelGGL(k_q80_quantize, dim3(ceil_div(blocks * 32, threads)), dim3(threads),
                       0, cur_stream(), x.data_ptr<float>(), q.data_ptr<int8_t>(),
                       s.data_ptr<float>(), bs.data_ptr<float>(), (int)blocks);
}

void rmsnorm(torch::Tensor x, torch::Tensor w, torch::Tensor y, double eps) {
    CHECK_CUDA(x);
    const int n = x.size(-1);
    const int rows = x.numel() / n;
    hipLaunchKernelGGL(k_rmsnorm, dim3(rows), dim3(256), 0, cur_stream(),
                       x.data_ptr<float>(), w.data_ptr<float>(), y.data_ptr<float>(),
                       n, (float)eps);
}

void rmsnorm_q80(torch::Tensor x, torch::Tensor w, torch::Tensor q,
                 torch::Tensor s, torch::Tensor bs, double eps) {
    CHECK_CUDA(x);
    const int n = x.size(-1);
    const int rows = x.numel() / n;
    hipLaunchKernelGGL(k_rmsnorm_q80, dim3(rows), dim3(256), 0, cur_stream(),
                       x.data_ptr<float>(), w.data_ptr<float>(), q.data_ptr<int8_t>(),
                       s.data_ptr<float>(), bs.data_ptr<float>(), n, (float)eps);
}

void rmsnorm_rows(torch::Tensor x, torch::Tensor w, torch::Tensor y, double eps) {
    CHECK_CUDA(x);
    const int hd = x.size(-1);
    const int rows = x.numel() / hd;
    hipLaunchKernelGGL(k_rmsnorm_rows, dim3(rows), dim3(64), 0, cur_stream(),
                       x.data_ptr<float>(), w.data_ptr<float>(), y.data_ptr<float>(),
                       hd, (float)eps);
}

void embed_gather(torch::Tensor table, torch::Tensor tokens, torch::Tensor x,
                  int64_t batch, c10::optional<torch::Tensor> ssq = c10::nullopt) {
    CHECK_CUDA(table);
    const int dim = table.size(1);
    const dim3 grid(ceil_div(dim / 4, 256), batch);
    hipLaunchKernelGGL(k_embed_gather, grid, dim3(256), 0, cur_stream(),
                       table.data_ptr<float>(), (const long *)tokens.data_ptr<int64_t>(),
                       x.data_ptr<float>(), dim,
                       ssq.has_value() ? ssq->data_ptr<float>() : nullptr);
}

void norm_quant(torch::Tensor x, torch::Tensor w, torch::Tensor ssq,
                torch::Tensor q, torch::Tensor s, torch::Tensor bs,
                int64_t batch, double eps,
                c10::optional<torch::Tensor> yout = c10::nullopt,
                bool deferred = false) {
    CHECK_CUDA(x);
    const int n = x.size(-1);
    const dim3 grid(ceil_div(n, 256), batch);
    hipLaunchKernelGGL(k_norm_quant, grid, dim3(256), 0, cur_stream(),
                       x.data_ptr<float>(), w.data_ptr<float>(), ssq.data_ptr<float>(),
                       q.data_ptr<int8_t>(), s.data_ptr<float>(), bs.data_ptr<float>(),
                       yout.has_value() ? yout->data_ptr<float>() : nullptr,
                       n, (float)eps, deferred ? 1 : 0);
}

void argmax_token(torch::Tensor token, torch::Tensor x, torch::Tensor scratch) {
    // two-stage argmax of flat f32 x into token[0] (TP greedy decode)
    CHECK_CUDA(x); CHECK_CONT(x);
    const int64_t n = x.numel();
    const int blocks = (int)std::min<int64_t>(scratch.numel(), ceil_div(n, 4096));
    auto *sp = reinterpret_cast<unsigned long long *>(scratch.data_ptr<int64_t>());
    hipLaunchKernelGGL(k_argmax_stage1, dim3(blocks), dim3(256), 0, cur_stream(),
                       x.data_ptr<float>(), n, sp);
    hipLaunchKernelGGL(k_token_from_argmax, dim3(1), dim3(1024), 0, cur_stream(),
                       (long *)token.data_ptr<int64_t>(), sp, blocks);
}

void norm_f32(torch::Tensor x, torch::Tensor w, torch::Tensor ssq,
              torch::Tensor y, int64_t batch, double eps) {
    CHECK_CUDA(x);
    const int n = x.size(-1);
    const dim3 grid(ceil_div(n / 4, 256), batch);
    hipLaunchKernelGGL(k_norm_f32, grid, dim3(256), 0, cur_stream(),
                       x.data_ptr<float>(), w.data_ptr<float>(), ssq.data_ptr<float>(),
                       y.data_ptr<float>(), n, (float)eps);
}

void add_ssq(torch::Tensor x, torch::Tensor p, torch::Tensor ssq, int64_t batch) {
    CHECK_CUDA(x);
    const int n = x.size(-1);
    const dim3 grid(ceil_div(n, 1024), batch);
    hipLaunchKernelGGL(k_add_ssq, grid, dim3(256), 0, cur_stream(),
                       x.data_ptr<float>(), p.data_ptr<float>(),
                       ssq.data_ptr<float>(), n);
}

void swiglu_q80(torch::Tensor a, torch::Tensor g, int64_t lda, int64_t n,
                int64_t rows, torch::Tensor q, torch::Tensor s, torch::Tensor bs,
                bool gelu = false) {
    CHECK_CUDA(a);
    const int64_t blocks = rows * (n / QB);
    if (gelu)
        hipLaunchKernelGGL(k_swiglu_q80<true>, dim3(ceil_div(blocks * 32, 256)),
                           dim3(256), 0, cur_stream(), a.data_ptr<float>(),
                           g.data_ptr<float>(), (int)lda, (int)n,
                           q.data_ptr<int8_t>(), s.data_ptr<float>(),
                           bs.data_ptr<float>(), (int)blocks);
    else
        hipLaunchKernelGGL(k_swiglu_q80<false>, dim3(ceil_div(blocks * 32, 256)),
                           dim3(256), 0, cur_stream(), a.data_ptr<float>(),
                           g.data_ptr<float>(), (int)lda, (int)n,
                           q.data_ptr<int8_t>(), s.data_ptr<float>(),
                           bs.data_ptr<float>(), (int)blocks);
}

void rmsnorm_rows_s(torch::Tensor buf, int64_t ld, int64_t off, int64_t heads,
                    int64_t batch, torch::Tensor w, int64_t hd, double eps) {
    CHECK_CUDA(buf);
    hipLaunchKernelGGL(k_rmsnorm_rows_s, dim3(batch * heads), dim3(64), 0,
                       cur_stream(), buf.data_ptr<float>(), (int)ld, (int)off,
                       (int)heads, w.data_ptr<float>(), (int)hd, (float)eps);
}

void add_rmsnorm(torch::Tensor x, c10::optional<torch::Tensor> partial,
                 torch::Tensor w, torch::Tensor y, double eps) {
    CHECK_CUDA(x);
    const int n = x.size(-1);
    const int rows = x.numel() / n;
    const bool add = partial.has_value();
    const float *pp = add ? partial->data_ptr<float>() : nullptr;
    if (add)
        hipLaunchKernelGGL((k_add_rmsnorm<true, false>), dim3(rows), dim3(1024),
                           n * 4, cur_stream(), x.data_ptr<float>(), pp, w.data_ptr<float>(),
                           y.data_ptr<float>(), nullptr, nullptr, nullptr, n, (float)eps);
    else
        hipLaunchKernelGGL((k_add_rmsnorm<false, false>), dim3(rows), dim3(1024),
                           n * 4, cur_stream(), x.data_ptr<float>(), pp, w.data_ptr<float>(),
                           y.data_ptr<float>(), nullptr, nullptr, nullptr, n, (float)eps);
}

void add_rmsnorm_q80(torch::Tensor x, c10::optional<torch::Tensor> partial,
                     torch::Tensor w, torch::Tensor q, torch::Tensor s,
                     torch::Tensor bs, double eps) {
    CHECK_CUDA(x);
    const int n = x.size(-1);
    const int rows = x.numel() / n;
    const bool add = partial.has_value();
    const float *pp = add ? partial->data_ptr<float>() : nullptr;
    if (add)
        hipLaunchKernelGGL((k_add_rmsnorm<true, true>), dim3(rows), dim3(1024),
                           n * 4, cur_stream(), x.data_ptr<float>(), pp, w.data_ptr<float>(),
                           nullptr, q.data_ptr<int8_t>(), s.data_ptr<float>(),
                           bs.data_ptr<float>(), n, (float)eps);
    else
        hipLaunchKernelGGL((k_add_rmsnorm<false, true>), dim3(rows), dim3(1024),
                           n * 4, cur_stream(), x.data_ptr<float>(), pp, w.data_ptr<float>(),
                           nullptr, q.data_ptr<int8_t>(), s.data_ptr<float>(),
                           bs.data_ptr<float>(), n, (float)eps);
}

void token_from_argmax(torch::Tensor token, torch::Tensor scratch, int64_t count) {
    hipLaunchKernelGGL(k_token_from_argmax, dim3(1), dim3(1024), 0, cur_stream(),
                       (long *)token.data_ptr<int64_t>(),
                       reinterpret_cast<unsigned long long *>(scratch.data_ptr<int64_t>()),
                       (int)count);
}

void silu_mul(torch::Tensor a, torch::Tensor g, torch::Tensor out) {
    CHECK_CUDA(a);
    const int64_t n = a.numel();
    hipLaunchKernelGGL(k_silu_mul, dim3(ceil_div(n, 256)), dim3(256), 0, cur_stream(),
                       a.data_ptr<float>(), g.data_ptr<float>(), out.data_ptr<float>(), n);
}

void add_(torch::Tensor x, torch::Tensor y) {
    CHECK_CUDA(x);
    hipLaunchKernelGGL(k_add, dim3(ceil_div(x.numel(), 256)), dim3(256), 0,
                       cur_stream(), x.data_ptr<float>(), y.data_ptr<float>(), x.numel());
}

void pos_inc(torch::Tensor pos, int64_t delta) {
    hipLaunchKernelGGL(k_inc, dim3(1), dim3(64), 0, cur_stream(),
                       pos.data_ptr<int>(), (int)delta);
}

void register_quant_norm(py::module &m) {
    m.def("q80_quantize", &q80_quantize);
    m.def("rmsnorm", &rmsnorm);
    m.def("rmsnorm_q80", &rmsnorm_q80);
    m.def("rmsnorm_rows", &rmsnorm_rows);
    m.def("rmsnorm_rows_s", &rmsnorm_rows_s);
    m.def("add_rmsnorm", &add_rmsnorm);
    m.def("add_rmsnorm_q80", &add_rmsnorm_q80);
    m.def("norm_quant", &norm_quant, py::arg("x"), py::arg("w"), py::arg("ssq"),
          py::arg("q"), py::arg("s"), py::arg("bs"), py::arg("batch"),
          py::arg("eps"), py::arg("yout") = py::none(),
          py::arg("deferred") = false);
    m.def("argmax_token", &argmax_token);
    m.def("norm_f32", &norm_f32);
    m.def("add_ssq", &add_ssq);
    m.def("embed_gather", &embed_gather, py::arg("table"), py::arg("tokens"), py::arg("x"), py::arg("batch"), py::arg("ssq") = py::none());
    m.def("swiglu_q80", &swiglu_q80, py::arg("a"), py::arg("g"),
          py::arg("lda"), py::arg("n"), py::arg("rows"), py::arg("q"),
          py::arg("s"), py::arg("bs"), py::arg("gelu") = false);
    m.def("silu_mul", &silu_mul);
    m.def("add_", &add_);
    m.def("pos_inc", &pos_inc);
    m.def("token_from_argmax", &token_from_argmax);
}
