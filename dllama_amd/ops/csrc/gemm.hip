// dllama_amd — int8 MFMA prefill GEMM.

#include "dllama_common.h"

// ------------------------------------------------- int8 MFMA prefill GEMM
// Batched (prefill) Q40xQ80 matmul on the matrix cores:
// C[b][m] = sum_j sw[m,j]*sx[b,j] * (x_i8[b, j*32..] . w_i4[m, j*32..])
// One v_mfma_i32_32x32x32_i8 per (32-row, 32-batch, 1-block) tile — K=32
// matches the quant block exactly, so per-block scales stay exact: the i32
// tile is descaled into f32 accumulators after every MFMA.
// Fragment layouts verified on-device (tools/mfma_probe.hip):
//   A[m][k]: lane=(m&31)|((k>>4)<<5), byte=k&15 ; B[k][n] mirrored on n;
//   C[m][n]: col=lane&31, row=(r&3)+8*(r>>2)+4*(lane>>5).
// Weights ride as the B operand so each lane needs only ONE weight-row
// scale per block; the 16 batch-row x-scales come from wave-private LDS.
typedef int v4i32_t __attribute__((ext_vector_type(4)));
typedef int v16i32_t __attribute__((ext_vector_type(16)));

__global__ void __launch_bounds__(256)
k_q40_gemm(const uint8_t *__restrict__ qs,
           const __half *__restrict__ scales,
           const int8_t *__restrict__ xq,
           const float *__restrict__ xs,
           float *__restrict__ y,
           float *__restrict__ part,
           int d, int n, int batch) {
    // gridDim.y = K-splits: a pure M decomposition leaves <1 workgroup/CU
    // for mid-size d (224 wg for the 28672-row W13) — K-split partials
    // restore occupancy, combined by k_gemm_reduce
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int mbase = (blockIdx.x * 4 + wave) * 32;  // 32 weight rows per wave
    if (mbase >= d) return;
    const int nb = n / QB;
    const int ksplit = gridDim.y;
    const int j0 = (int)((int64_t)nb * blockIdx.y / ksplit);
    const int j1 = (int)((int64_t)nb * (blockIdx.y + 1) / ksplit);
    const int khi = lane >> 5;       // 0: elems 0..15 (lo nibbles), 1: 16..31 (hi)
    const int bcol = lane & 31;      // x batch row for the A fragment
    const int mcol = lane & 31;      // weight row within the tile (B operand)
    const int mrow = min(mbase + mcol, d - 1);
    const uint4 *wrow = reinterpret_cast<const uint4 *>(qs + (int64_t)mrow * (n >> 1));
    const __half *srow = scales + (int64_t)mrow * nb;

    float facc[16];
    #pragma unroll
    for (int r = 0; r < 16; r++) facc[r] = 0.0f;

    // 2-block unroll: two independent load->MFMA->descale chains keep two
    // 16B weight loads in flight per lane (single-chain was latency-bound:
    // MfmaUtil 1.5%)
    auto extract = [&](const uint4 &wq, v4i32_t &b) {
        const uint32_t wv[4] = {wq.x, wq.y, wq.z, wq.w};
        #pragma unroll
        for (int t = 0; t < 4; t++) {
            uint32_t sx_ = khi ? ((wv[t] >> 4) & 0x0F0F0F0Fu)
                               : (wv[t] & 0x0F0F0F0Fu);
            sx_ ^= 0x08080808u;
            b[t] = (int)(sx_ | (((sx_ >> 3) & 0x01010101u) * 0xF0u));
        }
    };
    int j = j0;
    for (; j + 1 < j1; j += 2) {
        const float sxv0 = (lane < 32) ? xs[(int64_t)(lane & 31) * nb + j] : 0.0f;
        const float sxv1 = (lane < 32) ? xs[(int64_t)(lane & 31) * nb + j + 1] : 0.0f;
        const uint4 wq0 = wrow[j];
        const uint4 wq1 = wrow[j + 1];
        v4i32_t a0 = *reinterpret_cast<const v4i32_t *>(
            xq + (int64_t)bcol * n + j * QB + khi * 16);
        v4i32_t a1 = *reinterpret_cast<const v4i32_t *>(
            xq + (int64_t)bcol * n + (j + 1) * QB + khi * 16);
        v4i32_t b0, b1;
        extract(wq0, b0);
        extract(wq1, b1);
        v16i32_t i0 = {}, i1 = {};
        i0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, i0, 0, 0, 0);
        i1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, i1, 0, 0, 0);
        const float sw0 = __half2float(srow[j]);
        const float sw1 = __half2float(srow[j + 1]);
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const int brow = (r & 3) + 8 * (r >> 2) + 4 * khi;
            facc[r] = fmaf((float)i0[r], sw0 * __shfl(sxv0, brow, WAVE), facc[r]);
            facc[r] = fmaf((float)i1[r], sw1 * __shfl(sxv1, brow, WAVE), facc[r]);
        }
    }
    for (; j < j1; j++) {
        const float sxv = (lane < 32) ? xs[(int64_t)(lane & 31) * nb + j] : 0.0f;
        v4i32_t a = *reinterpret_cast<const v4i32_t *>(
            xq + (int64_t)bcol * n + j * QB + khi * 16);
        v4i32_t b;
        extract(wrow[j], b);
        v16i32_t iacc = {};
        iacc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, iacc, 0, 0, 0);
        const float sw = __half2float(srow[j]);
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const int brow = (r & 3) + 8 * (r >> 2) + 4 * khi;
            facc[r] = fmaf((float)iacc[r], sw * __shfl(sxv, brow, WAVE), facc[r]);
        }
    }
    if (mbase + mcol < d) {
        #pragma unroll
        for (int r = 0; r < 16; r++) {
            const int brow = (r & 3) + 8 * (r >> 2) + 4 * khi;
            if (ksplit == 1) {
                if (brow < batch)
                    y[(int64_t)brow * d + mbase + mcol] = facc[r];
            } else {
                part[(((int64_t)blockIdx.y * 32) + brow) * d + mbase + mcol] = facc[r];
            }
        }
    }
}

// The default prefill GEMM since round 2 (DLLAMA_GEMM_V2=0 reverts; see
// tools/gemm_v2_probe.hip for the standalone A/B harness). Differences vs
// the round-1 k_q40_gemm:
//   - activation fragments + x-scales staged in LDS per 8-block chunk,
//     loaded once per workgroup and shared by all 4 waves,
//   - weight uint4 tiles prefetched through a 4-deep register ring,
//   - descale as float2 pairs (adjacent C rows) with broadcast ds_reads.
// 71 VGPR + 16 AGPR (v1: 126+30) -> 5 waves/SIMD, no spills.
#define GEMM_V2_CHUNK 8

__global__ void __launch_bounds__(256)
k_q40_gemm_v2(const uint8_t *__restrict__ qs,
              const __half *__restrict__ scales,
              const int8_t *__restrict__ xq,
              const float *__restrict__ xs,
              float *__restrict__ y,
              float *__restrict__ part,
              int d, int n, int batch) {
    __shared__ int8_t lds_a[2][GEMM_V2_CHUNK][32][QB];
    __shared__ float lds_s[2][GEMM_V2_CHUNK][32];
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int tid = threadIdx.x;
    const int mbase = (blockIdx.x * 4 + wave) * 32;
    const int nb = n / QB;
    const int ksplit = gridDim.y;
    const int j0 = (int)((int64_t)nb * blockIdx.y / ksplit);
    const int j1 = (int)((int64_t)nb * (blockIdx.y + 1) / ksplit);
    const int khi = lane >> 5;
    const int mcol = lane & 31;
    const int mrow = min(mbase + mcol, d - 1);
    const uint4 *wrow = reinterpret_cast<const uint4 *>(qs + (int64_t)mrow * (n >> 1));
    const __half *srow = scales + (int64_t)mrow * nb;
    const bool live = mbase < d;

    auto stage = [&](int buf, int jc) {
        const int nblk = min(GEMM_V2_CHUNK, j1 - jc);
        for (int u = tid; u < nblk * 32; u += 256) {
            const int b = u & 31;
            const int blk = u >> 5;
            *reinterpret_cast<uint4 *>(&lds_a[buf][blk][b][0]) =
                *reinterpret_cast<const uint4 *>(xq + (int64_t)b * n + (jc + blk) * QB);
            *reinterpret_cast<uint4 *>(&lds_a[buf][blk][b][16]) =
                *reinterpret_cast<const uint4 *>(xq + (int64_t)b * n + (jc + blk) * QB + 16);
            lds_s[buf][blk][b] = xs[(int64_t)b * nb + (jc + blk)];
        }
    };
    auto extract = [&](const uint4 &wq, v4i32_t &b) {
        const uint32_t wv[4] = {wq.x, wq.y, wq.z, wq.w};
        #pragma unroll
        for (int t = 0; t < 4; t++) {
            uint32_t s = khi ? ((wv[t] >> 4) & 0x0F0F0F0Fu) : (wv[t] & 0x0F0F0F0Fu);
            s ^= 0x08080808u;
            b[t] = (int)(s | (((s >> 3) & 0x01010101u) * 0xF0u));
        }
    };

    float2 facc[8];
    #pragma unroll
    for (int r = 0; r < 8; r++) facc[r] = make_float2(0.0f, 0.0f);

    stage(0, j0);
    // weight pipeline as NAMED scalars (cur/next): an indexed prefetch ring
    // array gets allocated to scratch (80 B/lane round-trip in the hot
    // loop — final code-object metadata shows it even when -Rpass remarks
    // claim zero spill); two named uint4s cannot spill, and the compiler's
    // vmcnt counting still overlaps the next load with the current MFMA
    uint4 wq_cur = {};
    float sw_cur = 0.0f;
    if (live && j0 < j1) {
        wq_cur = wrow[j0];
        sw_cur = __half2float(srow[j0]);
    }
    __syncthreads();

    int buf = 0;
    for (int jc = j0; jc < j1; jc += GEMM_V2_CHUNK, buf ^= 1) {
        const int nblk = min(GEMM_V2_CHUNK, j1 - jc);
        if (jc + GEMM_V2_CHUNK < j1) stage(buf ^ 1, jc + GEMM_V2_CHUNK);
        if (live) {
            #pragma unroll
            for (int jj = 0; jj < GEMM_V2_CHUNK; jj++) {
                if (jj >= nblk) break;
                const int j = jc + jj;
                const uint4 wq = wq_cur;
                const float sw = sw_cur;
                if (j + 1 < j1) {
                    wq_cur = wrow[j + 1];
                    sw_cur = __half2float(srow[j + 1]);
                }
                v4i32_t a = *reinterpret_cast<const v4i32_t *>(
                    &lds_a[buf][jj][lane & 31][khi * 16]);
                v4i32_t b;
                extract(wq, b);
                v16i32_t iacc = {};
                iacc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, iacc, 0, 0, 0);
                #pragma unroll
                for (int r2 = 0; r2 < 8; r2++) {
                    const int brow = ((2 * r2) & 3) + 8 * (r2 >> 1) + 4 * khi;
                    const float2 sx2 = *reinterpret_cast<const float2 *>(
                        &lds_s[buf][jj][brow]);
                    facc[r2].x = fmaf((float)iacc[2 * r2], sw * sx2.x, facc[r2].x);
                    facc[r2].y = fmaf((float)iacc[2 * r2 + 1], sw * sx2.y, facc[r2].y);
                }
            }
        }
        __syncthreads();
    }

    if (live && mbase + mcol < d) {
        #pragma unroll
        for (int r2 = 0; r2 < 8; r2++) {
            const int brow = ((2 * r2) & 3) + 8 * (r2 >> 1) + 4 * khi;
            if (ksplit == 1) {
                if (brow < batch)
                    y[(int64_t)brow * d + mbase + mcol] = facc[r2].x;
                if (brow + 1 < batch)
                    y[(int64_t)(brow + 1) * d + mbase + mcol] = facc[r2].y;
            } else {
                part[(((int64_t)blockIdx.y * 32) + brow) * d + mbase + mcol] = facc[r2].x;
                part[(((int64_t)blockIdx.y * 32) + brow + 1) * d + mbase + mcol] = facc[r2].y;
            }
        }
    }
}

__global__ void k_gemm_reduce(const float *__restrict__ part,
                              float *__restrict__ y,
                              int d, int batch, int ksplit) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < (int64_t)batch * d; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / d);
        const int m = (int)(i % d);
        float acc = 0.0f;
        for (int k = 0; k < ksplit; k++)
            acc += part[(((int64_t)k * 32) + b) * d + m];
        y[(int64_t)b * d + m] = acc;
    }
}

// ============================================================== host bindings

void q40_gemm(torch::Tensor qs, torch::Tensor scales, torch::Tensor xq,
              torch::Tensor xs, torch::Tensor y, int64_t batch,
              c10::optional<torch::Tensor> part = c10::nullopt,
              int64_t variant = -1) {
    // int8-MFMA batched matmul (prefill path); xq/xs must have >=32 rows
    CHECK_CUDA(qs); CHECK_CONT(qs); CHECK_CONT(xq);
    const int d = qs.size(0);
    const int n = qs.size(1) * 2;
    TORCH_CHECK(xq.size(-1) == n, "x width mismatch");
    TORCH_CHECK(xq.size(0) >= 32, "gemm needs 32 padded batch rows");
    TORCH_CHECK(batch <= 32, "the MFMA fragment covers 32 batch rows; "
                "chunk larger prompts (rows past 32 would be dropped)");
    TORCH_CHECK(n % QB == 0, "n must be a multiple of 32");
    const int mtiles = ceil_div(d, 128);
    int ksplit = 1;
    if (part.has_value()) {
        ksplit = std::max(1, std::min(1024 / mtiles, 16));
        ksplit = std::min<int>(ksplit, n / QB);
        while (ksplit > 1 && (int64_t)ksplit * 32 * d > part->numel()) ksplit--;
    }
    float *pp = ksplit > 1 ? part->data_ptr<float>() : nullptr;
    // v2 (LDS-staged) is the default since round 2 (validated on hardware:
    // ~25% faster at all three prefill shapes); DLLAMA_GEMM_V2=0 reverts
    static const bool env_v2 = !std::getenv("DLLAMA_GEMM_V2")
        || atoi(std::getenv("DLLAMA_GEMM_V2")) != 0;
    const bool v2 = variant < 0 ? env_v2 : variant == 1;
    auto *kern = v2 ? k_q40_gemm_v2 : k_q40_gemm;
    hipLaunchKernelGGL(kern, dim3(mtiles, ksplit), dim3(256), 0,
                       cur_stream(), qs.data_ptr<uint8_t>(),
                       reinterpret_cast<const __half *>(scales.data_ptr<at::Half>()),
                       xq.data_ptr<int8_t>(), xs.data_ptr<float>(),
                       y.data_ptr<float>(), pp, d, n, (int)batch);
    if (ksplit > 1)
        hipLaunchKernelGGL(k_gemm_reduce, dim3(ceil_div((int64_t)batch * d, 256)),
                           dim3(256), 0, cur_stream(), pp, y.data_ptr<float>(),
                           d, (int)batch, ksplit);
}

void register_gemm(py::module &m) {
    m.def("q40_gemm", &q40_gemm, py::arg("qs"), py::arg("scales"),
          py::arg("xq"), py::arg("xs"), py::arg("y"), py::arg("batch"),
          py::arg("part") = py::none(), py::arg("variant") = -1);
}
