// dllama_amd — tensor-parallel Q80 wire: pack, merge-add and logits assembly.

#include "dllama_common.h"

// ------------------------------------------------------------------ q80 sync pack / merge-add
// wire layout per row: n int8 payload then n/32 f16 scales
// (role of cast-forward-f32-q80.comp; consumed after RCCL all-gather by
//  k_merge_add, the reference merge-add-forward-q80-f32.comp equivalent).
// fused quantize-into-wire: one pass replaces k_q80_quantize + k_sync_pack
// for the TP sync (the wire consumer k_merge_add needs no blocksum).
// The model's default; DLLAMA_FUSED_SYNC=0 splits it into the two kernels
// again.
__global__ void k_sync_quant_pack(const float *__restrict__ x,
                                  uint8_t *__restrict__ buf,
                                  int n, int n_blocks_total) {
    const int gid = (blockIdx.x * blockDim.x + threadIdx.x) / 32;
    const int lane = threadIdx.x & 31;
    if (gid >= n_blocks_total) return;
    const int nb = n / QB;
    const int r = gid / nb, jb = gid % nb;
    const int row_bytes = n + 2 * nb;
    uint8_t *row = buf + (int64_t)r * row_bytes;
    const Q80Lane c = q80_quant_group32(x[(int64_t)gid * QB + lane]);
    row[jb * QB + lane] = (uint8_t)(int8_t)c.qf;
    if (lane == 0) wire_store_scale(row, n, jb, c.d);
}

__global__ void k_sync_pack(const int8_t *__restrict__ q,
                            const float *__restrict__ s,
                            uint8_t *__restrict__ buf,
                            int n, int rows) {
    const int nb = n / QB;
    const int row_bytes = n + 2 * nb;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < (int64_t)rows * n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = i / n, c = i % n;
        uint8_t *row = buf + (int64_t)r * row_bytes;
        row[c] = (uint8_t)q[i];
        if (c < nb) wire_store_scale(row, n, c, s[(int64_t)r * nb + c]);
    }
}

// x[r, i] += sum_w dequant(bufs[w, r, i]) — the all-reduce completion
// (reference OP_MERGE_ADD, nn-cpu-ops.cpp:920-957).
__global__ void k_merge_add(float *__restrict__ x,
                            const uint8_t *__restrict__ bufs,
                            float *__restrict__ ssq,
                            int world, int n, int rows) {
    const int nb = n / QB;
    const int row_bytes = n + 2 * nb;
    const int r = blockIdx.y;
    float local = 0.0f;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n;
         c += gridDim.x * blockDim.x) {
        float acc = x[(int64_t)r * n + c];
        for (int w = 0; w < world; w++)
            acc = wire_load_fma(bufs + ((int64_t)w * rows + r) * row_bytes, n, c, acc);
        x[(int64_t)r * n + c] = acc;
        local += acc * acc;
    }
    if (ssq != nullptr) ssq_block_add<0>(ssq, r, local);
}

// merge_add + DEFERRED Q80 emit of x*wnorm (the next matmul's input; the
// PRO==2 consumer applies inv_rms): completes the TP all-reduce AND
// replaces the following norm_quant launch. One 256-thread wg per 256
// elements = 8 wg-local quant blocks.
__global__ void k_merge_add_q(float *__restrict__ x,
                              const uint8_t *__restrict__ bufs,
                              float *__restrict__ ssq,
                              const float *__restrict__ wnorm,
                              int8_t *__restrict__ oq,
                              float *__restrict__ os,
                              float *__restrict__ obs,
                              int world, int n, int rows) {
    const int nb = n / QB;
    const int row_bytes = n + 2 * nb;
    const int r = blockIdx.y;
    const int c = blockIdx.x * 256 + threadIdx.x;
    float acc = x[(int64_t)r * n + c];
    for (int w = 0; w < world; w++)
        acc = wire_load_fma(bufs + ((int64_t)w * rows + r) * row_bytes, n, c, acc);
    x[(int64_t)r * n + c] = acc;
    ssq_block_add<4>(ssq, r, acc * acc);
    const Q80Lane q = q80_quant_group32(acc * wnorm[c]);
    oq[(int64_t)r * n + c] = (int8_t)q.qf;
    const float bsum = group32_reduce_sum(q.qf);
    if ((threadIdx.x & 31) == 0) {
        os[(int64_t)r * nb + c / QB] = q.d;
        obs[(int64_t)r * nb + c / QB] = bsum;
    }
}

// TP logits assembly: the row-split wcls puts rank w's slice at global vocab
// offset w*vocab0, so full logits for batch row b are the concatenation of
// gather[w, b, :] over w (reference gathers the same slices to root,
// nn-network.cpp:568-600 with onlyFromWorkerToRoot). One strided copy kernel
// instead of a per-token ATen permute+reshape.
__global__ void k_logits_concat(float *__restrict__ dst,
                                const float *__restrict__ src,
                                int nb, int vocab0, int world) {
    const int b = blockIdx.y;
    const int64_t total = (int64_t)world * vocab0;
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int w = i / vocab0, j = i - (int64_t)w * vocab0;
        dst[(int64_t)b * total + i] =
            src[((int64_t)w * nb + b) * vocab0 + j];
    }
}

// ============================================================== host bindings

void logits_concat(torch::Tensor dst, torch::Tensor src, int64_t batch) {
    // src [world, nb, vocab0] (contiguous all-gather output) -> dst rows
    // 0..batch-1 of [.., world*vocab0]
    CHECK_CUDA(dst); CHECK_CONT(src);
    const int world = src.size(0);
    const int nb = src.size(1);
    const int vocab0 = src.size(2);
    const int64_t total = (int64_t)world * vocab0;
    hipLaunchKernelGGL(k_logits_concat,
                       dim3(std::min<int64_t>(ceil_div(total, 256), 2048), batch),
                       dim3(256), 0, cur_stream(), dst.data_ptr<float>(),
                       src.data_ptr<float>(), nb, vocab0, world);
}

void sync_pack(torch::Tensor q, torch::Tensor s, torch::Tensor buf) {
    CHECK_CUDA(q);
    const int n = q.size(-1);
    const int rows = q.numel() / n;
    hipLaunchKernelGGL(k_sync_pack, dim3(ceil_div((int64_t)rows * n, 256)), dim3(256),
                       0, cur_stream(), q.data_ptr<int8_t>(), s.data_ptr<float>(),
                       buf.data_ptr<uint8_t>(), n, rows);
}

void sync_quant_pack(torch::Tensor x, torch::Tensor buf) {
    CHECK_CUDA(x);
    const int n = x.size(-1);
    const int rows = x.numel() / n;
    const int blocks = rows * (n / QB);
    hipLaunchKernelGGL(k_sync_quant_pack, dim3(ceil_div(blocks * 32, 256)),
                       dim3(256), 0, cur_stream(), x.data_ptr<float>(),
                       buf.data_ptr<uint8_t>(), n, blocks);
}

void merge_add_q(torch::Tensor x, torch::Tensor bufs, torch::Tensor ssq,
                 torch::Tensor wnorm, torch::Tensor oq, torch::Tensor os,
                 torch::Tensor obs) {
    // bufs [world, rows, row_bytes] (all-gather output); x [rows, n]
    CHECK_CUDA(x); CHECK_CONT(bufs);
    const int world = bufs.size(0);
    const int rows = bufs.size(1);
    const int n = x.size(-1);
    TORCH_CHECK(n % 256 == 0, "merge_add_q needs dim % 256 == 0");
    hipLaunchKernelGGL(k_merge_add_q, dim3(n / 256, rows), dim3(256), 0,
                       cur_stream(), x.data_ptr<float>(),
                       bufs.data_ptr<uint8_t>(), ssq.data_ptr<float>(),
                       wnorm.data_ptr<float>(), oq.data_ptr<int8_t>(),
                       os.data_ptr<float>(), obs.data_ptr<float>(),
                       world, n, rows);
}

void merge_add(torch::Tensor x, torch::Tensor bufs,
               c10::optional<torch::Tensor> ssq = c10::nullopt) {
    CHECK_CUDA(x);
    const int n = x.size(-1);
    const int rows = x.numel() / n;
    const int world = bufs.size(0);
    hipLaunchKernelGGL(k_merge_add, dim3(ceil_div(n, 1024), rows), dim3(256),
                       0, cur_stream(), x.data_ptr<float>(), bufs.data_ptr<uint8_t>(),
                       ssq.has_value() ? ssq->data_ptr<float>() : nullptr,
                       world, n, rows);
}

void register_sync(py::module &m) {
    m.def("merge_add_q", &merge_add_q);
    m.def("logits_concat", &logits_concat);
    m.def("sync_pack", &sync_pack);
    m.def("sync_quant_pack", &sync_quant_pack);
    m.def("merge_add", &merge_add, py::arg("x"), py::arg("bufs"), py::arg("ssq") = py::none());
}
