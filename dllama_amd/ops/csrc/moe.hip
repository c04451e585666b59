// dllama_amd — MoE router, gate and expert-merge kernels.

#include "dllama_common.h"

// router GEMV with the FFN rmsnorm fused: logits[b][e] =
// inv_rms(b) * sum_i gate[e,i] * x[b,i] * wnorm[i] — the MoE deferred-quant
// path never materializes t_norm (reference computes rms_norm then the gate
// matmul as separate ops, llm.cpp:430-450)
__global__ void k_router_gemv_norm(const float *__restrict__ gate,
                                   const float *__restrict__ x,
                                   const float *__restrict__ wnorm,
                                   const float *__restrict__ ssq,
                                   float *__restrict__ logits,
                                   int n_experts, int dim, float eps) {
    const int e = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    const int b = blockIdx.y;
    if (e >= n_experts) return;
    const int lane = threadIdx.x % WAVE;
    const float inv = rsqrtf(ssq_total_wave(ssq, b, lane) / dim + eps);
    const float4 *g4 = reinterpret_cast<const float4 *>(gate + (int64_t)e * dim);
    const float4 *x4 = reinterpret_cast<const float4 *>(x + (int64_t)b * dim);
    const float4 *w4 = reinterpret_cast<const float4 *>(wnorm);
    float acc = 0.0f;
    for (int i = lane; i < dim / 4; i += WAVE) {
        const float4 gv = g4[i];
        const float4 xv = x4[i];
        const float4 wv = w4[i];
        acc += gv.x * xv.x * wv.x + gv.y * xv.y * wv.y
             + gv.z * xv.z * wv.z + gv.w * xv.w * wv.w;
    }
    acc = wave_reduce_sum(acc);
    if (lane == 0) logits[(int64_t)b * n_experts + e] = acc * inv;
}

// f32 router GEMV: logits[b][e] = gate[e,:] . t[b,:]
__global__ void k_router_gemv(const float *__restrict__ gate,
                              const float *__restrict__ t,
                              float *__restrict__ logits,
                              int n_experts, int dim) {
    const int e = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    const int b = blockIdx.y;
    if (e >= n_experts) return;
    const int lane = threadIdx.x % WAVE;
    const float4 *g4 = reinterpret_cast<const float4 *>(gate + (int64_t)e * dim);
    const float4 *t4 = reinterpret_cast<const float4 *>(t + (int64_t)b * dim);
    float acc = 0.0f;
    for (int i = lane; i < dim / 4; i += WAVE) {
        const float4 gv = g4[i];
        const float4 tv = t4[i];
        acc += gv.x * tv.x + gv.y * tv.y + gv.z * tv.z + gv.w * tv.w;
    }
    acc = wave_reduce_sum(acc);
    if (lane == 0) logits[(int64_t)b * n_experts + e] = acc;
}

// MoE router: softmax over n_experts logits, top-k (first-index ties),
// normalized weights + int32 expert ids (reference OP_SOFTMAX + OP_MOE_GATE,
// nn-cpu-ops.cpp:1443-1492). One wave per batch row; n_experts <= 1024.
// rank-select top-k (replaces the iterative wave-argmax version): expert
// e's output slot is its rank = #{j: p_j > p_e} + #{j < e: p_j == p_e}
// (identical ordering and smallest-index tie-break as the reference's
// insertion sort, nn-cpu-ops.cpp:900-916). All-pairs comparison is pure
// parallel VALU over LDS — the old 8 serial rounds of 6-step wave argmax
// were shuffle-latency-bound (~6 us wall for one wave; measured
// tools/fuse_shape_probe G-vs-F).
__global__ void k_moe_gate(const float *__restrict__ logits,
                           int *__restrict__ idx,
                           float *__restrict__ wts,
                           int n_experts, int topk) {
    const int b = blockIdx.x;
    const float *lrow = logits + (int64_t)b * n_experts;
    __shared__ float p[1024];
    __shared__ float red[16];
    __shared__ float topsum;
    const int t = threadIdx.x;           // blockDim == 128
    const int wid = t / WAVE, lane = t % WAVE;
    float m = -1e30f;
    for (int i = t; i < n_experts; i += blockDim.x) {
        const float v = lrow[i];
        p[i] = v;
        m = fmaxf(m, v);
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        m = fmaxf(m, __shfl_xor(m, off, WAVE));
    if (lane == 0) red[wid] = m;
    __syncthreads();
    m = fmaxf(red[0], red[1]);
    // softmax numerator only: the full-softmax denominator cancels in the
    // top-k normalization (w_t = p_t / sum_topk p)
    for (int i = t; i < n_experts; i += blockDim.x)
        p[i] = __expf(p[i] - m);
    if (t == 0) topsum = 0.0f;
    __syncthreads();
    for (int i = t; i < n_experts; i += blockDim.x) {
        const float mine = p[i];
        int rank = 0;
        for (int j = 0; j < n_experts; j++) {
            const float o = p[j];
            rank += (o > mine) || (o == mine && j < i);
        }
        if (rank < topk) {
            idx[(int64_t)b * topk + rank] = i;
            wts[(int64_t)b * topk + rank] = mine;  // normalized below
            atomicAdd(&topsum, mine);
        }
    }
    __syncthreads();
    if (t < topk)
        wts[(int64_t)b * topk + t] /= topsum;
}

// weighted sum of expert outputs + residual fold + ssq (reference OP_SCALE +
// OP_MERGE_SUM + merge_add fused): x[b] += sum_s wts[b,s] * y[b*k+s].
// GATE=true recomputes the expert weights from the router logits in-kernel
// (same deterministic moe_gate_wave as the grouped GEMVs).
template <bool GATE = false>
__global__ void k_scale_merge_add(float *__restrict__ x,
                                  const float *__restrict__ y,
                                  const float *__restrict__ wts,
                                  float *__restrict__ ssq,
                                  int n, int topk, int n_experts) {
    const int b = blockIdx.y;
    float gw[16];
    if constexpr (GATE) {
        int gi[16];
        moe_gate_wave(wts + (int64_t)b * n_experts, n_experts, topk,
                      threadIdx.x % WAVE, gi, gw);
    }
    float local = 0.0f;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gridDim.x * blockDim.x) {
        float acc = x[(int64_t)b * n + i];
        if constexpr (GATE) {
            #pragma unroll
            for (int s = 0; s < 16; s++)
                if (s < topk)
                    acc = fmaf(gw[s], y[((int64_t)b * topk + s) * n + i], acc);
        } else {
            for (int s = 0; s < topk; s++)
                acc = fmaf(wts[(int64_t)b * topk + s],
                           y[((int64_t)b * topk + s) * n + i], acc);
        }
        x[(int64_t)b * n + i] = acc;
        local += acc * acc;
    }
    ssq_block_add<0>(ssq, b, local);
}

// TP variant of the above: weighted expert sum into the partial buffer
// (no residual fold, no ssq — those happen after the Q80 sync merge-add;
// replaces the eager torch.sum fallback so TP MoE decode stays
// graph-capturable with zero ATen in the step)
template <bool GATE = false>
__global__ void k_scale_merge(float *__restrict__ partial,
                              const float *__restrict__ y,
                              const float *__restrict__ wts,
                              int n, int topk, int n_experts) {
    const int b = blockIdx.y;
    float gw[16];
    if constexpr (GATE) {
        int gi[16];
        moe_gate_wave(wts + (int64_t)b * n_experts, n_experts, topk,
                      threadIdx.x % WAVE, gi, gw);
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gridDim.x * blockDim.x) {
        float acc = 0.0f;
        if constexpr (GATE) {
            #pragma unroll
            for (int s = 0; s < 16; s++)
                if (s < topk)
                    acc = fmaf(gw[s], y[((int64_t)b * topk + s) * n + i], acc);
        } else {
            for (int s = 0; s < topk; s++)
                acc = fmaf(wts[(int64_t)b * topk + s],
                           y[((int64_t)b * topk + s) * n + i], acc);
        }
        partial[(int64_t)b * n + i] = acc;
    }
}

// MoE deferred-quant epilogue: weighted expert sum + residual fold + ssq +
// DEFERRED Q80 emit of x*wnorm (the next matmul's input; consumer applies
// inv_rms). Each 256-thread wg owns 256 consecutive elements = 8 wg-local
// Q80 blocks, so the quantization is barrier-free per 32-lane group.
__global__ void k_scale_merge_add_q(float *__restrict__ x,
                                    const float *__restrict__ y,
                                    const float *__restrict__ wts,
                                    float *__restrict__ ssq,
                                    const float *__restrict__ wnorm,
                                    int8_t *__restrict__ oq,
                                    float *__restrict__ os,
                                    float *__restrict__ obs,
                                    int n, int topk) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    float acc = x[(int64_t)b * n + i];
    for (int s = 0; s < topk; s++)
        acc = fmaf(wts[(int64_t)b * topk + s],
                   y[((int64_t)b * topk + s) * n + i], acc);
    x[(int64_t)b * n + i] = acc;
    ssq_block_add<4>(ssq, b, acc * acc);
    // deferred quant of x*wnorm: block = this thread's 32-lane group
    const Q80Lane c = q80_quant_group32(acc * wnorm[i]);
    oq[(int64_t)b * n + i] = (int8_t)c.qf;
    const float bsum = group32_reduce_sum(c.qf);
    if ((threadIdx.x & 31) == 0) {
        const int blk = i / QB;
        os[(int64_t)b * (n / QB) + blk] = c.d;
        obs[(int64_t)b * (n / QB) + blk] = bsum;
    }
}

// TP MoE epilogue: expert-weighted sum of the grouped-GEMV outputs packed
// straight into the Q80 wire (the all-gather payload) — replaces
// scale_merge + sync_quant_pack on the TP critical path. One 256-thread wg
// per 256 elements (8 wire blocks), B=1 decode.
__global__ void k_scale_merge_pack(const float *__restrict__ y,
                                   const float *__restrict__ wts,
                                   uint8_t *__restrict__ buf,
                                   int n, int topk) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    float acc = 0.0f;
    for (int s = 0; s < topk; s++)
        acc = fmaf(wts[(int64_t)b * topk + s],
                   y[((int64_t)b * topk + s) * n + i], acc);
    const Q80Lane c = q80_quant_group32(acc);
    const int row_bytes = n + 2 * (n / QB);
    uint8_t *row = buf + (int64_t)b * row_bytes;
    row[i] = (uint8_t)(int8_t)c.qf;
    if ((threadIdx.x & 31) == 0) wire_store_scale(row, n, i / QB, c.d);
}

// ============================================================== host bindings

void moe_gate(torch::Tensor logits, torch::Tensor idx, torch::Tensor wts,
              int64_t batch, int64_t topk) {
    CHECK_CUDA(logits);
    const int n_experts = logits.size(-1);
    TORCH_CHECK(n_experts <= 1024, "moe_gate supports <=1024 experts");
    hipLaunchKernelGGL(k_moe_gate, dim3(batch), dim3(128), 0, cur_stream(),
                       logits.data_ptr<float>(), idx.data_ptr<int>(),
                       wts.data_ptr<float>(), n_experts, (int)topk);
}

void scale_merge_add(torch::Tensor x, torch::Tensor y, torch::Tensor wts,
                     torch::Tensor ssq, int64_t batch, int64_t topk,
                     bool gate = false) {
    // gate=true: wts is the [B, n_experts] router-logits buffer and the
    // expert weights are recomputed in-kernel
    CHECK_CUDA(x);
    const int n = x.size(-1);
    const int ne = gate ? (int)wts.size(-1) : 0;
    auto launch = [&](auto k) {
        hipLaunchKernelGGL(k, dim3(ceil_div(n, 256), batch), dim3(256),
                           0, cur_stream(), x.data_ptr<float>(), y.data_ptr<float>(),
                           wts.data_ptr<float>(), ssq.data_ptr<float>(), n,
                           (int)topk, ne);
    };
    if (gate) launch(k_scale_merge_add<true>);
    else launch(k_scale_merge_add<false>);
}

void scale_merge(torch::Tensor partial, torch::Tensor y, torch::Tensor wts,
                 int64_t batch, int64_t topk, bool gate = false) {
    CHECK_CUDA(partial);
    const int n = partial.size(-1);
    const int ne = gate ? (int)wts.size(-1) : 0;
    auto launch = [&](auto k) {
        hipLaunchKernelGGL(k, dim3(ceil_div(n, 256), batch), dim3(256),
                           0, cur_stream(), partial.data_ptr<float>(),
                           y.data_ptr<float>(), wts.data_ptr<float>(), n,
                           (int)topk, ne);
    };
    if (gate) launch(k_scale_merge<true>);
    else launch(k_scale_merge<false>);
}

void scale_merge_add_q(torch::Tensor x, torch::Tensor y, torch::Tensor wts,
                       torch::Tensor ssq, torch::Tensor wnorm,
                       torch::Tensor oq, torch::Tensor os, torch::Tensor obs,
                       int64_t batch, int64_t topk) {
    CHECK_CUDA(x);
    const int n = x.size(-1);
    TORCH_CHECK(n % 256 == 0, "scale_merge_add_q needs dim % 256 == 0");
    hipLaunchKernelGGL(k_scale_merge_add_q, dim3(n / 256, batch), dim3(256),
                       0, cur_stream(), x.data_ptr<float>(), y.data_ptr<float>(),
                       wts.data_ptr<float>(), ssq.data_ptr<float>(),
                       wnorm.data_ptr<float>(), oq.data_ptr<int8_t>(),
                       os.data_ptr<float>(), obs.data_ptr<float>(), n, (int)topk);
}

void router_gemv_norm(torch::Tensor gate, torch::Tensor x, torch::Tensor wnorm,
                      torch::Tensor ssq, double eps, torch::Tensor logits,
                      int64_t batch) {
    CHECK_CUDA(gate);
    const int n_experts = gate.size(0);
    const int dim = gate.size(1);
    hipLaunchKernelGGL(k_router_gemv_norm, dim3(ceil_div(n_experts, 4), batch),
                       dim3(256), 0, cur_stream(), gate.data_ptr<float>(),
                       x.data_ptr<float>(), wnorm.data_ptr<float>(),
                       ssq.data_ptr<float>(), logits.data_ptr<float>(),
                       n_experts, dim, (float)eps);
}

void router_gemv(torch::Tensor gate, torch::Tensor t, torch::Tensor logits,
                 int64_t batch) {
    CHECK_CUDA(gate);
    const int n_experts = gate.size(0);
    const int dim = gate.size(1);
    hipLaunchKernelGGL(k_router_gemv, dim3(ceil_div(n_experts, 4), batch),
                       dim3(256), 0, cur_stream(), gate.data_ptr<float>(),
                       t.data_ptr<float>(), logits.data_ptr<float>(),
                       n_experts, dim);
}

void scale_merge_pack(torch::Tensor y, torch::Tensor wts, torch::Tensor wire,
                      int64_t batch, int64_t topk, int64_t n) {
    CHECK_CUDA(y);
    TORCH_CHECK(n % 256 == 0, "scale_merge_pack needs dim % 256 == 0");
    hipLaunchKernelGGL(k_scale_merge_pack, dim3(n / 256, batch), dim3(256), 0,
                       cur_stream(), y.data_ptr<float>(), wts.data_ptr<float>(),
                       wire.data_ptr<uint8_t>(), (int)n, (int)topk);
}

void register_moe(py::module &m) {
    m.def("scale_merge_pack", &scale_merge_pack);
    m.def("moe_gate", &moe_gate);
    m.def("scale_merge_add", &scale_merge_add, py::arg("x"), py::arg("y"),
          py::arg("wts"), py::arg("ssq"), py::arg("batch"), py::arg("topk"),
          py::arg("gate") = false);
    m.def("scale_merge", &scale_merge, py::arg("partial"), py::arg("y"),
          py::arg("wts"), py::arg("batch"), py::arg("topk"),
          py::arg("gate") = false);
    m.def("router_gemv", &router_gemv);
    m.def("router_gemv_norm", &router_gemv_norm);
    m.def("scale_merge_add_q", &scale_merge_add_q);
}
