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

// ------------------------------------------- expert-grouped GEMM (MoE steps)
// The MoE matmul of a multi-row step, expert by expert: k_moe_group (moe.hip)
// has sorted the step's (row, k) slots by expert into tiles of at most 32
// slots of one expert, and a workgroup here computes one tile against 128
// weight rows of that expert, so an expert's weights are read once per step
// however many rows chose it (k_q40_gemv_grouped streams the expert once per
// slot, on the VALU).
//
// Work split: grid (ceil(d / 128), moe_max_tiles). grid.y is the routing-
// independent bound, so a captured step replays for any routing; a workgroup
// at or past the live tile count leaves on a uniform branch. Wave w owns 32
// weight rows of the expert in the stacked [E, rows, n/2] planes, the tile's
// slots are the MFMA N dimension: one v_mfma_i32_32x32x32_i8 per Q40 block
// and chain, descaled by sw * sx into f32 exactly as k_q40_gemm_v2 does
// (K = 32 is the quantisation block, so the per-block scales stay exact).
//
// Activations are gathered: column c of the tile is slot perm[first + c] and
// reads input row slot / k_slots (k_slots = topk where the slots of a row
// share it, 1 where every slot has a row of its own). Thread t stages block
// t / 32 of column t % 32 of an 8-block chunk: loaded into registers before
// the chunk's MFMAs and written to the other LDS buffer after them, shared
// by the 4 waves. A column at or past `count` is staged as zero codes with a
// zero scale and no address is formed for it. Columns never mix: a slot's
// result does not depend on what shares its tile.
//
// Weights come through a 4-block register ring, three loads ahead of the
// MFMA (the comment at the ring says why it is not v2's cur/next pair).
//
// Epilogues. GEPI_PLAIN stores f32 y[slot][row] for c < count. GEPI_SILU /
// GEPI_GELU (d = ff, ff % 32 == 0): the wave also owns rows ff + m .. of the
// same expert (W3 under W1), two independent MFMA chains per block on one A
// fragment, forms act(a) * g in registers as k_swiglu_q80 computes it, and
// emits the Q80 triple [S, ff]: in the C layout the 32 lanes of a half-wave
// hold one slot's 32 consecutive ff indices, one Q80 block.
//
// No K-split: at Qwen3-30B-A3B shapes a 32-row chunk already launches about
// 12 x 112 (W1|W3) and 16 x 112 (W2) live workgroups on 256 CUs.
enum { GEPI_PLAIN = 0, GEPI_SILU = 1, GEPI_GELU = 2 };
#define GEMM_GROUPED_RING 4
static_assert(GEMM_V2_CHUNK % GEMM_GROUPED_RING == 0, "ring indices are per-chunk constants");

template <int EPI>
__global__ void __launch_bounds__(256)
k_q40_gemm_grouped(const uint8_t *__restrict__ qs,
                   const __half *__restrict__ scales,
                   const int8_t *__restrict__ xq,
                   const float *__restrict__ xs,
                   const int *__restrict__ plan,
                   float *__restrict__ y,
                   int8_t *__restrict__ oq,
                   float *__restrict__ os,
                   float *__restrict__ obs,
                   int d, int n, int n_experts, int n_slots, int k_slots) {
    constexpr bool SWIGLU = EPI != GEPI_PLAIN;
    __shared__ int8_t lds_a[2][GEMM_V2_CHUNK][MOE_TILE][QB];
    __shared__ float lds_s[2][GEMM_V2_CHUNK][MOE_TILE];
    __shared__ int lds_slot[MOE_TILE];  // slot of column c, -1 past count
    const int tile = blockIdx.y;
    if (tile >= plan[0]) return;  // workgroup-uniform
    const int *tp = plan + MOE_PLAN_TILES + 3 * tile;
    // a plan is trusted for its order, not for memory safety: the expert
    // and the columns are clamped to what the buffers hold
    const int e = min(max(tp[0], 0), n_experts - 1);
    const int first = max(tp[1], 0);
    const int count = min(min(tp[2], MOE_TILE), n_slots - first);

    const int tid = threadIdx.x;
    const int wave = tid / WAVE;
    const int lane = tid % WAVE;
    const int khi = lane >> 5;
    const int mcol = lane & 31;
    const int mbase = (blockIdx.x * 4 + wave) * 32;
    const bool live = mbase < d;  // wave-uniform
    const int mrow = min(mbase + mcol, d - 1);
    const int nb = n / QB;
    // the expert's planes hold W1 over W3 in the SwiGLU form
    const int64_t row_a = (int64_t)e * (SWIGLU ? 2 * d : d) + mrow;
    const uint4 *wrow_a = reinterpret_cast<const uint4 *>(qs + row_a * (n >> 1));
    const __half *srow_a = scales + row_a * nb;
    const uint4 *wrow_g = wrow_a + (int64_t)d * (n >> 5);  // d rows of n/32 uint4
    const __half *srow_g = srow_a + (int64_t)d * nb;

    // this thread's share of every staged chunk: block sblk of column scol
    const int scol = tid & 31;
    const int sblk = tid >> 5;
    const int my_slot = scol < count ? plan[MOE_PLAN_PERM + first + scol] : -1;
    if (tid < MOE_TILE) lds_slot[tid] = my_slot;
    uint4 sa0, sa1;
    float ssx;
    auto stage_load = [&](int jc) {
        sa0 = make_uint4(0, 0, 0, 0);
        sa1 = sa0;
        ssx = 0.0f;
        if (my_slot >= 0 && jc + sblk < nb) {
            const int64_t xr = my_slot / k_slots;
            const uint4 *p = reinterpret_cast<const uint4 *>(
                xq + xr * n + (jc + sblk) * QB);
            sa0 = p[0];
            sa1 = p[1];
            ssx = xs[xr * nb + jc + sblk];
        }
    };
    auto stage_store = [&](int buf) {
        *reinterpret_cast<uint4 *>(&lds_a[buf][sblk][scol][0]) = sa0;
        *reinterpret_cast<uint4 *>(&lds_a[buf][sblk][scol][16]) = sa1;
        lds_s[buf][sblk][scol] = ssx;
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

    float2 fa[8], fg[8];
    #pragma unroll
    for (int r = 0; r < 8; r++) {
        fa[r] = make_float2(0.0f, 0.0f);
        fg[r] = make_float2(0.0f, 0.0f);
    }

    stage_load(0);
    stage_store(0);
    // weights: a ring of GEMM_GROUPED_RING blocks per chain, RING - 1 loads
    // in flight ahead of the MFMA. The chunk loop below is fully unrolled
    // and a chunk is a multiple of the ring, so every ring index is a
    // compile-time constant and the ring lives in registers (v2's note on
    // ring arrays is about a runtime index). With v2's single block ahead a
    // wave paid one memory latency per block: at MoE shapes few workgroups
    // share a CU and nothing else hides it.
    uint4 wa_ring[GEMM_GROUPED_RING], wg_ring[GEMM_GROUPED_RING];
    __half swa_ring[GEMM_GROUPED_RING], swg_ring[GEMM_GROUPED_RING];
    #pragma unroll
    for (int i = 0; i < GEMM_GROUPED_RING; i++) {
        wa_ring[i] = wg_ring[i] = make_uint4(0, 0, 0, 0);
        swa_ring[i] = swg_ring[i] = __float2half(0.0f);
        if (live && i < GEMM_GROUPED_RING - 1 && i < nb) {
            wa_ring[i] = wrow_a[i];
            swa_ring[i] = srow_a[i];
            if constexpr (SWIGLU) {
                wg_ring[i] = wrow_g[i];
                swg_ring[i] = srow_g[i];
            }
        }
    }
    __syncthreads();

    int buf = 0;
    for (int jc = 0; jc < nb; jc += GEMM_V2_CHUNK, buf ^= 1) {
        const int nblk = min(GEMM_V2_CHUNK, nb - jc);
        const bool more = jc + GEMM_V2_CHUNK < nb;
        if (more) stage_load(jc + GEMM_V2_CHUNK);
        if (live) {
            #pragma unroll
            for (int jj = 0; jj < GEMM_V2_CHUNK; jj++) {
                if (jj >= nblk) break;
                const int j = jc + jj;
                constexpr int R = GEMM_GROUPED_RING;
                const uint4 wa = wa_ring[jj % R], wg = wg_ring[jj % R];
                const float swa = __half2float(swa_ring[jj % R]);
                const float swg = __half2float(swg_ring[jj % R]);
                if (j + R - 1 < nb) {
                    wa_ring[(jj + R - 1) % R] = wrow_a[j + R - 1];
                    swa_ring[(jj + R - 1) % R] = srow_a[j + R - 1];
                    if constexpr (SWIGLU) {
                        wg_ring[(jj + R - 1) % R] = wrow_g[j + R - 1];
                        swg_ring[(jj + R - 1) % R] = srow_g[j + R - 1];
                    }
                }
                const v4i32_t a = *reinterpret_cast<const v4i32_t *>(
                    &lds_a[buf][jj][lane & 31][khi * 16]);
                v4i32_t b;
                extract(wa, b);
                v16i32_t ia = {}, ig = {};
                ia = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, ia, 0, 0, 0);
                if constexpr (SWIGLU) {
                    extract(wg, b);
                    ig = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, ig, 0, 0, 0);
                }
                #pragma unroll
                for (int r2 = 0; r2 < 8; r2++) {
                    const int col = ((2 * r2) & 3) + 8 * (r2 >> 1) + 4 * khi;
                    const float2 sx2 = *reinterpret_cast<const float2 *>(
                        &lds_s[buf][jj][col]);
                    // single-lane ops: v2's float2 descale compiles to
                    // packed f32 VALU ops, which this kernel keeps out
                    fa[r2].x = fma_f32((float)ia[2 * r2], mul_f32(swa, sx2.x), fa[r2].x);
                    fa[r2].y = fma_f32((float)ia[2 * r2 + 1], mul_f32(swa, sx2.y), fa[r2].y);
                    if constexpr (SWIGLU) {
                        fg[r2].x = fma_f32((float)ig[2 * r2], mul_f32(swg, sx2.x), fg[r2].x);
                        fg[r2].y = fma_f32((float)ig[2 * r2 + 1], mul_f32(swg, sx2.y), fg[r2].y);
                    }
                }
            }
        }
        if (more) stage_store(buf ^ 1);
        __syncthreads();
    }

    if (!live) return;
    const int m = mbase + mcol;
    #pragma unroll
    for (int r = 0; r < 16; r++) {
        const int col = (r & 3) + 8 * (r >> 2) + 4 * khi;
        const int slot = lds_slot[col];
        const float av = (r & 1) ? fa[r >> 1].y : fa[r >> 1].x;
        if constexpr (!SWIGLU) {
            if (slot >= 0 && m < d) y[(int64_t)slot * d + m] = av;
        } else {
            // d % 32 == 0: every lane of a live wave holds a row, and the
            // half-wave's 32 rows are Q80 block mbase / 32 of the slot
            const float gv = (r & 1) ? fg[r >> 1].y : fg[r >> 1].x;
            // silu or tanh-approx gelu, the expressions of k_swiglu_q80
            const float act = EPI == GEPI_GELU
                ? 0.5f * av * (1.0f + tanhf(0.797884560802865f * (av + 0.044715f * av * av * av)))
                : av / (1.0f + __expf(-av));
            const Q80Lane c = q80_quant_group32(act * gv);
            const float bsum = group32_reduce_sum(c.qf);
            if (slot >= 0) {
                oq[(int64_t)slot * d + m] = (int8_t)c.qf;
                if (mcol == 0) {
                    os[(int64_t)slot * (d / QB) + mbase / QB] = c.d;
                    obs[(int64_t)slot * (d / QB) + mbase / QB] = bsum;
                }
            }
        }
    }
}

// ------------------------------------ weight-streaming GEMM (1..32-row steps)
// The Q40xQ80 product for 1..32 activation rows as one launch that reads the
// weights in whole cache lines (opt-in: DLLAMA_GEMM_STREAM, docs/DESIGN.md
// §12). v_mfma_i32_16x16x32_i8 with the weights as the A operand: one MFMA
// is 16 weight rows x 16 activation rows (columns) x one Q40 block, NT column
// tiles share the A fragment. Fragment layout (tests/test_gemm_stream.py runs
// asymmetric inputs through it): A lane = m + 16 g holds k-group g of row m,
// B mirrored on the column, C register r of that lane is row 4 g + r of
// column m. k-group g is block elements 4g..4g+3 and 16+4g..16+4g+3: the lo
// and hi nibbles of dword g of the block, so the unpack is and / shift / and
// and the nibbles stay unsigned. The -8 offset rides in as the MFMA's C
// input, -8 * bsum[col][block], the same in a lane's four registers.
//
// Work split. A workgroup owns RT row tiles (16 or 32 weight rows), its W
// waves split K in chunks of 8 blocks, contiguous chunk ranges per wave. Each
// wave accumulates its slice in f32 (descale sw * sx rounded once, then one
// fma per block, in block order), the W partial tiles are summed through LDS
// in wave order, and the first RT * NT waves store the result: no K-split
// across workgroups, no scratch buffer, no second launch. RT and W come from
// (d, n) alone (stream_shape), so a row's bits depend neither on `batch` nor
// on NT.
//
// Load path: through wave-private LDS tiles, not an in-register exchange.
// A load instruction takes 8 weight rows x 8 blocks: 8 lanes hold the 8
// consecutive 16-byte blocks of one row, one whole 128-byte line. The MFMA
// wants dword g of block j of row m in lane m + 16 g, a 4 x 16 transpose of
// dwords across all four 16-lane rows of the wave; permlane16/32 swaps move
// whole rows pairwise and would need two swap rounds plus selects per block
// per tile, against one ds_write_b128 per 8 blocks and one ds_read_b32 per
// block here, and the same tile serves the activations: read directly in
// fragment order they are 16 bytes of 16 different lines per load (16 tag
// look-ups for 256 bytes), staged they are 256 contiguous bytes per 16 lanes.
// The block index is XOR-swizzled with the row inside a tile so that both the
// b128 writes and the b32 fragment reads touch every bank once. The tiles
// are wave-private: a wave reads only what it wrote, in program order, so
// the K loop has no barrier.
//
// Weights (the HBM stream) come through a 4-chunk register ring, issued
// three chunks ahead; the chunk loop is unrolled by the ring so every ring
// index is a compile-time constant. Activation codes, their scales and the
// weight scales (L2 hits) are loaded one chunk ahead, before the ring's load
// in program order, so waiting for them does not drain the ring.
//
// Activation bytes per weight byte, from L2: a chunk is RT * 2 KiB of
// weights and min(batch, 16 NT) * 256 B of codes, i.e. batch / (8 RT):
// 1 at 8 rows, 2 at 16 and 4 at 32 for RT = 1, half that for RT = 2.
//
// Edges: rows at or past d are clamped for loads and masked at the store;
// columns at or past `batch` are staged as zero codes and form no address;
// blocks at or past n / 32 are neither loaded nor multiplied.
//
// GS_PLAIN stores f32 y[b][row]; GS_RESID folds the residual like
// q40_gemv_resid: x[b][row] += y and the squares into ssq_slot(b, blockIdx.x).
enum { GS_PLAIN = 0, GS_RESID = 1 };
#define GS_CHUNK 8
#define GS_RING 4
typedef uint4 __attribute__((may_alias)) gs_uint4;
typedef uint2 __attribute__((may_alias)) gs_uint2;
typedef float4 __attribute__((may_alias)) gs_float4;

// dwords of LDS per wave: weight tile, code tile, weight scales, {sx, -8 bsum}
static constexpr int gs_wave_dwords(int NT, int RT) {
    return RT * 512 + NT * 1024 + RT * 128 + NT * 256;
}

__device__ __forceinline__ float add_f32(float a, float b) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

template <int NT, int RT, int EPI>
__global__ void __launch_bounds__(512)
k_q40_gemm_stream(const uint8_t *__restrict__ qs,
                  const __half *__restrict__ scales,
                  const int8_t *__restrict__ xq,
                  const float *__restrict__ xs,
                  const float *__restrict__ xbs,
                  float *__restrict__ y,    // GS_RESID: the residual x
                  float *__restrict__ ssq,  // GS_RESID only
                  int d, int n, int batch) {
    extern __shared__ uint32_t gs_lds[];
    constexpr int WD = gs_wave_dwords(NT, RT);
    constexpr int R = GS_RING;
    const int tid = threadIdx.x;
    const int W = blockDim.x / WAVE;
    const int wave = tid / WAVE;
    const int lane = tid % WAVE;
    const int m = lane & 15;   // fragment row (A) / column (B, C)
    const int g = lane >> 4;   // k-group; C rows 4g..4g+3
    const int lrow = lane >> 3;  // staging: row (or column) within 8
    const int lblk = lane & 7;   // staging: block of the chunk
    uint32_t *wl = gs_lds + wave * WD;
    uint32_t *xl = wl + RT * 512;
    float *swl = reinterpret_cast<float *>(xl + NT * 1024);
    uint32_t *sbl = xl + NT * 1024 + RT * 128;

    const int nb = n / QB;
    const int nchunks = (nb + GS_CHUNK - 1) / GS_CHUNK;
    const int c0 = nchunks * wave / W;
    const int c1 = nchunks * (wave + 1) / W;
    const int rbase = blockIdx.x * (RT * 16);

    // staging addresses: load i takes rows rbase + 8 i .. + 7
    const uint4 *wp[RT * 2];
    const __half *sp[RT * 2];
    int wst[RT * 2];
    #pragma unroll
    for (int i = 0; i < RT * 2; i++) {
        const int row = min(rbase + i * 8 + lrow, d - 1);
        wp[i] = reinterpret_cast<const uint4 *>(qs + (int64_t)row * (n >> 1)) + lblk;
        sp[i] = scales + (int64_t)row * nb + lblk;
        const int r16 = (i & 1) * 8 + lrow;
        wst[i] = i * 256 + lrow * 32 + ((lblk ^ ((r16 >> 1) & 7)) << 2);
    }
    // codes: uint4 u of column 4 q + g (of tile nt), 16 uint4 per chunk row
    const int xu = lane & 15;

    uint4 wr[R][RT * 2];
    uint4 xr[NT * 4];
    __half swr[RT * 2];
    float sxr[NT * 2], bsr[NT * 2];

    auto load_w = [&](uint4 (&slot)[RT * 2], int c) {
        const bool ok = c * GS_CHUNK + lblk < nb;
        #pragma unroll
        for (int i = 0; i < RT * 2; i++)
            slot[i] = ok ? wp[i][c * GS_CHUNK] : make_uint4(0, 0, 0, 0);
    };
    auto load_x = [&](int c) {
        const bool okb = c * GS_CHUNK + lblk < nb;
        #pragma unroll
        for (int i = 0; i < RT * 2; i++)
            swr[i] = okb ? sp[i][c * GS_CHUNK] : __float2half(0.0f);
        #pragma unroll
        for (int i = 0; i < NT * 2; i++) {
            const int col = i * 8 + lrow;
            const bool ok = okb && col < batch;
            const int64_t at = (int64_t)col * nb + c * GS_CHUNK + lblk;
            sxr[i] = ok ? xs[at] : 0.0f;
            bsr[i] = ok ? xbs[at] : 0.0f;
        }
        const bool oku = c * GS_CHUNK + (xu >> 1) < nb;
        #pragma unroll
        for (int i = 0; i < NT * 4; i++) {
            const int col = (i >> 2) * 16 + (i & 3) * 4 + g;
            xr[i] = make_uint4(0, 0, 0, 0);
            if (oku && col < batch)
                xr[i] = *reinterpret_cast<const uint4 *>(
                    xq + (int64_t)col * n + (int64_t)c * (GS_CHUNK * QB) + xu * 16);
        }
    };
    auto stage = [&](const uint4 (&slot)[RT * 2]) {
        #pragma unroll
        for (int i = 0; i < RT * 2; i++) {
            *reinterpret_cast<gs_uint4 *>(wl + wst[i]) = slot[i];
            swl[lblk * (RT * 16) + i * 8 + lrow] = __half2float(swr[i]);
        }
        #pragma unroll
        for (int i = 0; i < NT * 2; i++) {
            const int col = i * 8 + lrow;
            // the code sum is an integer below 2^24: exact in f32 and in int
            *reinterpret_cast<gs_uint2 *>(sbl + (lblk * (NT * 16) + col) * 2) =
                make_uint2(__float_as_uint(sxr[i]), (uint32_t)(-8 * (int)bsr[i]));
        }
        #pragma unroll
        for (int i = 0; i < NT * 4; i++) {
            const int c16 = (i & 3) * 4 + g;
            *reinterpret_cast<gs_uint4 *>(
                xl + (i >> 2) * 1024 + c16 * 64 + ((xu ^ c16) << 2)) = xr[i];
        }
    };

    float acc[RT][NT][4];
    #pragma unroll
    for (int a = 0; a < RT; a++)
        #pragma unroll
        for (int b = 0; b < NT; b++)
            #pragma unroll
            for (int r = 0; r < 4; r++) acc[a][b][r] = 0.0f;

    if (c0 < c1) load_x(c0);
    #pragma unroll
    for (int i = 0; i < R - 1; i++) {
        if (c0 + i < c1) load_w(wr[i], c0 + i);
    }

    const int wrd = m * 32 + g;            // weight fragment read, + swizzled block
    const int wsw = (m >> 1) & 7;
    const int xrd = m * 64 + g;            // code fragment read
    auto block = [&](int jj) {
        long a[RT];
        gs_float4 sw4[RT];
        #pragma unroll
        for (int t = 0; t < RT; t++) {
            const uint32_t v = wl[t * 512 + wrd + ((jj ^ wsw) << 2)];
            const uint32_t lo = v & 0x0F0F0F0Fu;
            const uint32_t hi = (v >> 4) & 0x0F0F0F0Fu;
            a[t] = (long)(((uint64_t)hi << 32) | lo);
            sw4[t] = *reinterpret_cast<const gs_float4 *>(
                swl + jj * (RT * 16) + t * 16 + 4 * g);
        }
        #pragma unroll
        for (int u = 0; u < NT; u++) {
            const uint32_t x0 = xl[u * 1024 + xrd + (((2 * jj) ^ m) << 2)];
            const uint32_t x1 = xl[u * 1024 + xrd + (((2 * jj + 1) ^ m) << 2)];
            const long b = (long)(((uint64_t)x1 << 32) | x0);
            const gs_uint2 sb = *reinterpret_cast<const gs_uint2 *>(
                sbl + (jj * (NT * 16) + u * 16 + m) * 2);
            const float sx = __uint_as_float(sb.x);
            const int off = (int)sb.y;
            #pragma unroll
            for (int t = 0; t < RT; t++) {
                v4i32_t ci = {off, off, off, off};
                ci = __builtin_amdgcn_mfma_i32_16x16x32_i8(a[t], b, ci, 0, 0, 0);
                const float s4[4] = {sw4[t].x, sw4[t].y, sw4[t].z, sw4[t].w};
                #pragma unroll
                for (int r = 0; r < 4; r++)
                    acc[t][u][r] = fma_f32((float)ci[r], mul_f32(s4[r], sx),
                                           acc[t][u][r]);
            }
        }
    };
    for (int cb = c0; cb < c1; cb += R) {
        #pragma unroll
        for (int ii = 0; ii < R; ii++) {
            const int c = cb + ii;
            if (c >= c1) break;  // wave-uniform
            stage(wr[ii]);
            if (c + 1 < c1) load_x(c + 1);
            if (c + R - 1 < c1) load_w(wr[(ii + R - 1) % R], c + R - 1);
            const int nblk = min(GS_CHUNK, nb - c * GS_CHUNK);
            // a whole chunk runs as straight-line code, so the scheduler
            // overlaps the blocks' LDS reads, MFMAs and descales (in two
            // halves for the 4-tile form, which spilled as one)
            if (nblk == GS_CHUNK) {
                constexpr int UN = RT * NT == 4 ? GS_CHUNK / 2 : GS_CHUNK;
                #pragma unroll 1
                for (int j0 = 0; j0 < GS_CHUNK; j0 += UN) {
                    #pragma unroll
                    for (int q = 0; q < UN; q++) block(j0 + q);
                }
            } else {
                #pragma unroll 1
                for (int jj = 0; jj < nblk; jj++) block(jj);
            }
        }
    }

    // the W partial tiles, summed in wave order by the first RT * NT waves
    __syncthreads();
    gs_float4 *red = reinterpret_cast<gs_float4 *>(gs_lds);
    #pragma unroll
    for (int t = 0; t < RT; t++)
        #pragma unroll
        for (int u = 0; u < NT; u++)
            red[(wave * (RT * NT) + t * NT + u) * WAVE + lane] =
                make_float4(acc[t][u][0], acc[t][u][1], acc[t][u][2], acc[t][u][3]);
    __syncthreads();
    float sq = 0.0f;
    if (wave < RT * NT) {
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int w = 0; w < W; w++) {
            const gs_float4 p = red[(w * (RT * NT) + wave) * WAVE + lane];
            s[0] = add_f32(s[0], p.x);
            s[1] = add_f32(s[1], p.y);
            s[2] = add_f32(s[2], p.z);
            s[3] = add_f32(s[3], p.w);
        }
        const int col = (wave % NT) * 16 + m;
        const int row0 = rbase + (wave / NT) * 16 + 4 * g;
        if (col < batch) {
            #pragma unroll
            for (int r = 0; r < 4; r++) {
                if (row0 + r >= d) continue;
                float *at = y + (int64_t)col * d + row0 + r;
                if constexpr (EPI == GS_PLAIN) {
                    *at = s[r];
                } else {
                    const float xv = add_f32(*at, s[r]);
                    *at = xv;
                    sq = fma_f32(xv, xv, sq);
                }
            }
        }
    }
    if constexpr (EPI == GS_RESID) {
        // a column's squares: over the 4 k-groups by shuffle, over the RT row
        // tiles through LDS (past the partial tiles), one atomic per column
        float *sql = reinterpret_cast<float *>(gs_lds) + W * (RT * NT) * 256;
        sq += __shfl_xor(sq, 16, WAVE);
        sq += __shfl_xor(sq, 32, WAVE);
        if (wave < RT * NT && lane < 16) sql[wave * 16 + lane] = sq;
        __syncthreads();
        if (tid < NT * 16 && tid < batch) {
            float t = 0.0f;
            #pragma unroll
            for (int a = 0; a < RT; a++)
                t += sql[(a * NT + (tid >> 4)) * 16 + (tid & 15)];
            atomicAdd(ssq_slot(ssq, tid, blockIdx.x), t);
        }
    }
}

// -------------------------------------- LDS-tiled GEMM (prompt chunks, <= 128)
// The Q40xQ80 product for 1..128 activation rows, built around an activation
// tile instead of a weight stream (opt-in: prefill_rows, docs/DESIGN.md §14).
// A workgroup of 8 waves owns RT * 16 weight rows against ALL `batch`
// activation rows and walks K in chunks of 8 blocks; a chunk of both operands
// is staged in LDS once and read by every wave, so a weight byte leaves HBM
// once per call and an activation byte leaves L2 once per workgroup.
//
// MFMA, fragment layout, unpack, the -8 * bsum C input and the descale are
// k_q40_gemm_stream's (v_mfma_i32_16x16x32_i8, weights as A, 16 activation
// rows as the B columns): sw * sx rounded once, one f32 fma per block into the
// accumulator, in block order. No K split at all: one wave sums all n / 32
// blocks of its C tiles, so a row's bits depend on nothing but (n, the row).
//
// Work split, from (d, n) alone: RT = 1 (16 weight rows) below d = 6144, so
// that d = 4096 still launches 256 workgroups, RT = 2 from there. The 8 waves
// split the C tile, not K: wave w owns row tile w / (8 / RT) and the RT
// column tiles w % (8 / RT) + u * (8 / RT). `batch` enters only as the number
// of live 16-column tiles nt = ceil(batch / 16): a wave skips the MFMAs of a
// tile at or past nt, and LDS holds nt code tiles.
//
// LDS, per stage (two stages, dwords): weight tile RT * 512, code tiles
// nt * 1024, weight scales as f32 RT * 128, {sx, -8 bsum} nt * 256; in all
// 2 * (2.5 RT + 5 nt) KiB: 85 KiB at RT = 1 and 90 KiB at RT = 2 for 128 rows
// (one workgroup = 2 waves per SIMD on a CU of 160 KiB), 45 / 50 KiB for 64
// rows. There LDS would hold three workgroups but the registers decide: at
// 120..122 VGPRs (RT = 1) a SIMD holds 4 waves, two workgroups per CU; at
// 138..140 (RT = 2) it holds 3, which is one workgroup of 2 waves per SIMD
// again. Both tiles use §12's XOR swizzle unchanged: 8 lanes
// write the 8 blocks of one weight row (one 128-byte line) as b128, 16 lanes
// the 16 uint4 of one column's chunk; the b32 fragment reads touch every bank
// once. The tiles are shared now, so the K loop has one barrier per chunk:
// chunk c + 1 is loaded into registers before chunk c's MFMAs and written to
// the other stage after them.
//
// Edges as §12: rows at or past d are clamped for loads and masked at the
// store; columns at or past `batch` are staged as zeros and form no address;
// blocks at or past n / 32 are neither loaded nor multiplied.
//
// GT_PLAIN stores f32 y[b][row]; GT_RESID adds into x[b][row] in place and
// adds the column's squares, summed over the workgroup's rows, with one atomic
// per column into ssq_slot(b, blockIdx.x). `vec4`: d % 4 == 0 and a 16-byte
// aligned output, so a lane's four consecutive rows go as one 16-byte access.
enum { GT_PLAIN = 0, GT_RESID = 1 };
#define GT_CHUNK 8
#define GT_WAVES 8
#define GT_MAX_ROWS 128

// dwords of one LDS stage with nt live 16-column tiles
static constexpr int gt_stage_dwords(int RT, int nt) {
    return RT * 512 + nt * 1024 + RT * 128 + nt * 256;
}

template <int RT, int EPI>
__global__ void __launch_bounds__(GT_WAVES * WAVE)
k_q40_gemm_tile(const uint8_t *__restrict__ qs,
                const __half *__restrict__ scales,
                const int8_t *__restrict__ xq,
                const float *__restrict__ xs,
                const float *__restrict__ xbs,
                float *__restrict__ y,    // GT_RESID: the residual x
                float *__restrict__ ssq,  // GT_RESID only
                int d, int n, int batch, int vec4) {
    extern __shared__ uint32_t gt_lds[];
    constexpr int CG = GT_WAVES / RT;  // waves per row tile
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int lane = tid % WAVE;
    const int m = lane & 15;   // fragment row (A) / column (B, C)
    const int g = lane >> 4;   // k-group; C rows 4g..4g+3
    const int nt = (batch + 15) >> 4;
    const int ncols = nt * 16;
    const int SD = gt_stage_dwords(RT, nt);
    const int xoff = RT * 512, swoff = xoff + nt * 1024, sboff = swoff + RT * 128;
    const int nb = n / QB;
    const int nchunks = (nb + GT_CHUNK - 1) / GT_CHUNK;
    const int rbase = blockIdx.x * (RT * 16);
    const int rt = wave / CG;  // this wave's row tile
    const int cw = wave % CG;  // and its first column tile

    // staging roles. Weights: thread t < RT * 128 takes block t & 7 of row
    // t >> 3 of every chunk, and that row's scale of the block
    const int lblk = tid & 7;
    const int wrow = tid >> 3;
    const bool wrole = tid < RT * 128;
    const int grow = min(rbase + min(wrow, RT * 16 - 1), d - 1);
    const uint4 *wp = reinterpret_cast<const uint4 *>(qs + (int64_t)grow * (n >> 1)) + lblk;
    const __half *sp = scales + (int64_t)grow * nb + lblk;
    const int wst = wrow * 32 + ((lblk ^ ((wrow >> 1) & 7)) << 2);
    // codes: uint4 xu of the chunk of column 32 i + cb; {sx, bsum}: block
    // lblk of column 64 i + wrow
    const int xu = tid & 15;
    const int cb = tid >> 4;

    uint4 wr = make_uint4(0, 0, 0, 0);
    __half swr = __float2half(0.0f);
    uint4 xr[4];
    float sxr[2], bsr[2];

    auto load = [&](int c) {
        const bool okb = c * GT_CHUNK + lblk < nb;
        if (wrole) {
            wr = okb ? wp[c * GT_CHUNK] : make_uint4(0, 0, 0, 0);
            swr = okb ? sp[c * GT_CHUNK] : __float2half(0.0f);
        }
        #pragma unroll
        for (int i = 0; i < 2; i++) {
            const int col = i * 64 + wrow;
            const bool ok = okb && col < batch;
            const int64_t at = (int64_t)col * nb + c * GT_CHUNK + lblk;
            sxr[i] = ok ? xs[at] : 0.0f;
            bsr[i] = ok ? xbs[at] : 0.0f;
        }
        const bool oku = c * GT_CHUNK + (xu >> 1) < nb;
        #pragma unroll
        for (int i = 0; i < 4; i++) {
            const int col = i * 32 + cb;
            xr[i] = make_uint4(0, 0, 0, 0);
            if (oku && col < batch)
                xr[i] = *reinterpret_cast<const uint4 *>(
                    xq + (int64_t)col * n + (int64_t)c * (GT_CHUNK * QB) + xu * 16);
        }
    };
    auto stage = [&](int buf) {
        uint32_t *st = gt_lds + buf * SD;
        if (wrole) {
            *reinterpret_cast<gs_uint4 *>(st + wst) = wr;
            reinterpret_cast<float *>(st + swoff)[lblk * (RT * 16) + wrow] =
                __half2float(swr);
        }
        #pragma unroll
        for (int i = 0; i < 2; i++) {
            const int col = i * 64 + wrow;
            // the code sum is an integer below 2^24: exact in f32 and in int
            if (col < ncols)
                *reinterpret_cast<gs_uint2 *>(st + sboff + (lblk * ncols + col) * 2) =
                    make_uint2(__float_as_uint(sxr[i]), (uint32_t)(-8 * (int)bsr[i]));
        }
        #pragma unroll
        for (int i = 0; i < 4; i++) {
            const int col = i * 32 + cb;
            const int c16 = col & 15;
            if (col < ncols)
                *reinterpret_cast<gs_uint4 *>(
                    st + xoff + (col >> 4) * 1024 + c16 * 64 + ((xu ^ c16) << 2)) = xr[i];
        }
    };

    float acc[RT][4];
    bool live[RT];
    #pragma unroll
    for (int u = 0; u < RT; u++) {
        live[u] = cw + u * CG < nt;  // wave-uniform
        #pragma unroll
        for (int r = 0; r < 4; r++) acc[u][r] = 0.0f;
    }

    const int wrd = rt * 512 + m * 32 + g;  // weight fragment read, + swizzled block
    const int wsw = (m >> 1) & 7;
    const int xrd = xoff + m * 64 + g;      // code fragment read
    auto block = [&](const uint32_t *st, int jj) {
        const uint32_t v = st[wrd + ((jj ^ wsw) << 2)];
        const uint32_t lo = v & 0x0F0F0F0Fu;
        const uint32_t hi = (v >> 4) & 0x0F0F0F0Fu;
        const long a = (long)(((uint64_t)hi << 32) | lo);
        const gs_float4 sw4 = *reinterpret_cast<const gs_float4 *>(
            reinterpret_cast<const float *>(st + swoff) + jj * (RT * 16) + rt * 16 + 4 * g);
        const float s4[4] = {sw4.x, sw4.y, sw4.z, sw4.w};
        #pragma unroll
        for (int u = 0; u < RT; u++) {
            if (!live[u]) continue;
            const int tile = cw + u * CG;
            const uint32_t x0 = st[tile * 1024 + xrd + (((2 * jj) ^ m) << 2)];
            const uint32_t x1 = st[tile * 1024 + xrd + (((2 * jj + 1) ^ m) << 2)];
            const long b = (long)(((uint64_t)x1 << 32) | x0);
            const gs_uint2 sb = *reinterpret_cast<const gs_uint2 *>(
                st + sboff + (jj * ncols + tile * 16 + m) * 2);
            const float sx = __uint_as_float(sb.x);
            const int off = (int)sb.y;
            v4i32_t ci = {off, off, off, off};
            ci = __builtin_amdgcn_mfma_i32_16x16x32_i8(a, b, ci, 0, 0, 0);
            #pragma unroll
            for (int r = 0; r < 4; r++)
                acc[u][r] = fma_f32((float)ci[r], mul_f32(s4[r], sx), acc[u][r]);
        }
    };

    load(0);
    stage(0);
    __syncthreads();
    for (int c = 0; c < nchunks; c++) {
        const uint32_t *st = gt_lds + (c & 1) * SD;
        const bool more = c + 1 < nchunks;
        if (more) load(c + 1);
        const int nblk = min(GT_CHUNK, nb - c * GT_CHUNK);
        if (nblk == GT_CHUNK) {
            #pragma unroll
            for (int jj = 0; jj < GT_CHUNK; jj++) block(st, jj);
        } else {
            #pragma unroll 1
            for (int jj = 0; jj < nblk; jj++) block(st, jj);
        }
        // the other stage was last read before the previous barrier
        if (more) stage((c + 1) & 1);
        __syncthreads();
    }

    float sq[RT];
    const int row0 = rbase + rt * 16 + 4 * g;
    #pragma unroll
    for (int u = 0; u < RT; u++) {
        sq[u] = 0.0f;
        const int col = (cw + u * CG) * 16 + m;
        if (!live[u] || col >= batch || row0 >= d) continue;
        float *at = y + (int64_t)col * d + row0;
        if (vec4) {
            gs_float4 *at4 = reinterpret_cast<gs_float4 *>(at);
            if constexpr (EPI == GT_PLAIN) {
                *at4 = make_float4(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
            } else {
                gs_float4 xv = *at4;
                xv.x = add_f32(xv.x, acc[u][0]);
                xv.y = add_f32(xv.y, acc[u][1]);
                xv.z = add_f32(xv.z, acc[u][2]);
                xv.w = add_f32(xv.w, acc[u][3]);
                *at4 = xv;
                sq[u] = fma_f32(xv.x, xv.x, sq[u]);
                sq[u] = fma_f32(xv.y, xv.y, sq[u]);
                sq[u] = fma_f32(xv.z, xv.z, sq[u]);
                sq[u] = fma_f32(xv.w, xv.w, sq[u]);
            }
        } else {
            #pragma unroll
            for (int r = 0; r < 4; r++) {
                if (row0 + r >= d) continue;
                if constexpr (EPI == GT_PLAIN) {
                    at[r] = acc[u][r];
                } else {
                    const float xv = add_f32(at[r], acc[u][r]);
                    at[r] = xv;
                    sq[u] = fma_f32(xv, xv, sq[u]);
                }
            }
        }
    }
    if constexpr (EPI == GT_RESID) {
        // a column's squares: over the 4 k-groups by shuffle, over the RT row
        // tiles through LDS (the stages are dead: the K loop ended on a
        // barrier), one atomic per column and workgroup. Every live column
        // tile has exactly one wave per row tile.
        float *sql = reinterpret_cast<float *>(gt_lds);
        #pragma unroll
        for (int u = 0; u < RT; u++) {
            float s = sq[u];
            s += __shfl_xor(s, 16, WAVE);
            s += __shfl_xor(s, 32, WAVE);
            if (live[u] && g == 0)
                sql[rt * GT_MAX_ROWS + (cw + u * CG) * 16 + m] = s;
        }
        __syncthreads();
        if (tid < batch) {
            float t = 0.0f;
            #pragma unroll
            for (int a = 0; a < RT; a++) t += sql[a * GT_MAX_ROWS + tid];
            atomicAdd(ssq_slot(ssq, tid, blockIdx.x), t);
        }
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

void q40_gemm_grouped(torch::Tensor qs, torch::Tensor scales, torch::Tensor xq,
                      torch::Tensor xs, torch::Tensor plan, int64_t n_slots,
                      int64_t k_slots,
                      c10::optional<torch::Tensor> y = c10::nullopt,
                      c10::optional<torch::Tensor> oq = c10::nullopt,
                      c10::optional<torch::Tensor> os = c10::nullopt,
                      c10::optional<torch::Tensor> obs = c10::nullopt,
                      bool gelu = false) {
    // qs [E, rows, n/2] stacked expert planes; plan from moe_group over the
    // step's n_slots slots; slot s reads input row s / k_slots.
    // y given: plain form, rows = d, y f32 [n_slots, d].
    // oq/os/obs given: SwiGLU form, rows = 2 * ff (W1 over W3), the Q80
    // triple [n_slots, ff] of act(w1 x) * (w3 x).
    CHECK_CUDA(qs); CHECK_CONT(qs); CHECK_CONT(scales); CHECK_CONT(xq);
    CHECK_CONT(xs); CHECK_CUDA(plan); CHECK_CONT(plan);
    TORCH_CHECK(qs.dim() == 3, "grouped gemm takes stacked [E, rows, n/2] planes");
    const bool swiglu = oq.has_value();
    TORCH_CHECK(swiglu != y.has_value(), "pass y or the Q80 output triple");
    TORCH_CHECK(!swiglu || (os.has_value() && obs.has_value()),
                "the SwiGLU form writes oq, os and obs");
    const int n_experts = qs.size(0);
    const int rows = qs.size(1);
    const int n = qs.size(2) * 2;
    const int d = swiglu ? rows / 2 : rows;
    TORCH_CHECK(n >= QB && n % QB == 0, "n must be a multiple of 32");
    TORCH_CHECK(xq.size(-1) == n, "x width mismatch");
    TORCH_CHECK(n_slots >= 1 && n_slots <= MOE_PLAN_MAX_SLOTS,
                "grouped gemm supports 1..512 slots per step");
    TORCH_CHECK(k_slots >= 1 && xq.size(0) * k_slots >= n_slots
                && xs.numel() * QB >= xq.size(0) * (int64_t)n,
                "input triple shorter than n_slots / k_slots rows");
    TORCH_CHECK(plan.scalar_type() == torch::kInt32
                && plan.numel() >= MOE_PLAN_INTS, "moe plan buffer too small");
    const dim3 grid(ceil_div(d, 128), moe_max_tiles(n_experts, (int)n_slots));
    auto launch = [&](auto k, float *yp, int8_t *qp, float *sp, float *bp) {
        hipLaunchKernelGGL(k, grid, dim3(256), 0, cur_stream(),
                           qs.data_ptr<uint8_t>(),
                           reinterpret_cast<const __half *>(scales.data_ptr<at::Half>()),
                           xq.data_ptr<int8_t>(), xs.data_ptr<float>(),
                           plan.data_ptr<int>(), yp, qp, sp, bp, d, n,
                           n_experts, (int)n_slots, (int)k_slots);
    };
    if (!swiglu) {
        TORCH_CHECK(y->numel() >= n_slots * d, "y shorter than [n_slots, d]");
        launch(k_q40_gemm_grouped<GEPI_PLAIN>, y->data_ptr<float>(), nullptr,
               nullptr, nullptr);
        return;
    }
    TORCH_CHECK(rows % 2 == 0 && d % QB == 0,
                "the SwiGLU form needs ff % 32 == 0");
    TORCH_CHECK(oq->numel() >= n_slots * d && os->numel() * QB >= n_slots * d
                && obs->numel() * QB >= n_slots * d,
                "Q80 output shorter than [n_slots, ff]");
    if (gelu)
        launch(k_q40_gemm_grouped<GEPI_GELU>, nullptr, oq->data_ptr<int8_t>(),
               os->data_ptr<float>(), obs->data_ptr<float>());
    else
        launch(k_q40_gemm_grouped<GEPI_SILU>, nullptr, oq->data_ptr<int8_t>(),
               os->data_ptr<float>(), obs->data_ptr<float>());
}

// Rows per workgroup (16 or 32) and K-splitting waves (4 or 8) of the stream
// GEMM over a [d, n] matrix, from (d, n) alone so that a row's summation
// order does not depend on the batch. Measured with `tools/kernel_bench.py
// stream --sweep` at the 8B shapes (profiles/r16_stream_gemm.md): 16-row
// workgroups win at d = 4096 (wo, w2: 256 workgroups of 8 waves, two waves
// on every SIMD of 256 CUs), 32-row ones from d = 6144 up; 8 K-splitting
// waves win while the grid has at most two workgroups per CU, 4 above that
// (w13, wcls), and a wave is not given less than a chunk of 8 blocks.
// `rows` / `waves` override the rule: that is how the sweep runs.
struct StreamShape { int rt, waves; };

static StreamShape stream_shape(int d, int n, int rows, int waves) {
    StreamShape s;
    s.rt = rows ? rows / 16 : (d >= 6144 ? 2 : 1);
    const bool few = ceil_div(d, s.rt * 16) <= 512;
    s.waves = waves ? waves
        : (few && ceil_div(n / QB, GS_CHUNK) >= 8 ? 8 : 4);
    return s;
}

template <int NT, int RT, int EPI>
static void stream_launch(const StreamShape &s, const uint8_t *qs, const __half *sc,
                          const int8_t *xq, const float *xs, const float *xbs,
                          float *y, float *ssq, int d, int n, int batch) {
    auto *kern = k_q40_gemm_stream<NT, RT, EPI>;
    // 8 waves of the largest form stage 120 KiB, above the default cap
    static const hipError_t attr = hipFuncSetAttribute(
        reinterpret_cast<const void *>(kern),
        hipFuncAttributeMaxDynamicSharedMemorySize,
        8 * gs_wave_dwords(NT, RT) * 4);
    TORCH_CHECK(attr == hipSuccess, "stream gemm: LDS attribute: ",
                hipGetErrorString(attr));
    const size_t lds = (size_t)s.waves * gs_wave_dwords(NT, RT) * 4;
    hipLaunchKernelGGL(kern, dim3(ceil_div(d, RT * 16)), dim3(s.waves * WAVE),
                       lds, cur_stream(), qs, sc, xq, xs, xbs, y, ssq, d, n, batch);
}

template <int EPI>
static void stream_dispatch(torch::Tensor &qs, torch::Tensor &scales,
                            torch::Tensor &xq, torch::Tensor &xs,
                            torch::Tensor &xbs, torch::Tensor &y, float *ssq,
                            int64_t batch, int64_t rows, int64_t waves) {
    CHECK_CUDA(qs); CHECK_CONT(qs); CHECK_CONT(scales); CHECK_CONT(xq);
    CHECK_CONT(xs); CHECK_CONT(xbs); CHECK_CUDA(y); CHECK_CONT(y);
    const int d = qs.size(0);
    const int n = qs.size(1) * 2;
    TORCH_CHECK(d >= 1 && n >= QB && n % QB == 0, "n must be a multiple of 32");
    TORCH_CHECK(batch >= 1 && batch <= 32, "stream gemm takes 1..32 rows");
    TORCH_CHECK(xq.size(-1) == n && xq.numel() >= batch * n
                && xs.numel() * QB >= batch * n && xbs.numel() * QB >= batch * n,
                "input triple shorter than [batch, n]");
    TORCH_CHECK(xs.scalar_type() == torch::kFloat32
                && xbs.scalar_type() == torch::kFloat32
                && y.scalar_type() == torch::kFloat32, "xs, xbs and y are f32");
    TORCH_CHECK(y.numel() >= batch * d, "output shorter than [batch, d]");
    TORCH_CHECK((rows == 0 || rows == 16 || rows == 32)
                && (waves == 0 || waves == 4 || waves == 8),
                "stream gemm: rows 0/16/32, waves 0/4/8");
    const StreamShape s = stream_shape(d, n, (int)rows, (int)waves);
    auto go = [&](auto launch) {
        launch(s, qs.data_ptr<uint8_t>(),
               reinterpret_cast<const __half *>(scales.data_ptr<at::Half>()),
               xq.data_ptr<int8_t>(), xs.data_ptr<float>(), xbs.data_ptr<float>(),
               y.data_ptr<float>(), ssq, d, n, (int)batch);
    };
    if (batch <= 16) {
        if (s.rt == 1) go(stream_launch<1, 1, EPI>);
        else go(stream_launch<1, 2, EPI>);
    } else {
        if (s.rt == 1) go(stream_launch<2, 1, EPI>);
        else go(stream_launch<2, 2, EPI>);
    }
}

void q40_gemm_stream(torch::Tensor qs, torch::Tensor scales, torch::Tensor xq,
                     torch::Tensor xs, torch::Tensor xbs, torch::Tensor y,
                     int64_t batch, int64_t rows = 0, int64_t waves = 0) {
    // y f32 [batch, d] = the Q40 x Q80 product of the first `batch` rows
    stream_dispatch<GS_PLAIN>(qs, scales, xq, xs, xbs, y, nullptr, batch, rows, waves);
}

void q40_gemm_stream_resid(torch::Tensor qs, torch::Tensor scales,
                           torch::Tensor xq, torch::Tensor xs, torch::Tensor xbs,
                           torch::Tensor x, torch::Tensor ssq, int64_t batch,
                           int64_t rows = 0, int64_t waves = 0) {
    // x[b] += product, the rows' squares into ssq's spread slots
    CHECK_CUDA(ssq); CHECK_CONT(ssq);
    TORCH_CHECK(ssq.scalar_type() == torch::kFloat32
                && ssq.numel() >= batch * SSQ_SPREAD * SSQ_PAD,
                "ssq shorter than `batch` rows of spread slots");
    stream_dispatch<GS_RESID>(qs, scales, xq, xs, xbs, x, ssq.data_ptr<float>(),
                              batch, rows, waves);
}

// Weight rows per workgroup of the tiled GEMM over a [d, n] matrix, in tiles
// of 16, from d alone (a row's bits depend on neither): 16 rows keep 256
// workgroups at d = 4096 (wo, w2), 32 rows halve the activation re-reads from
// L2 wherever that still leaves more workgroups than CUs.
static int tile_rt(int d) { return d >= 6144 ? 2 : 1; }

template <int RT, int EPI>
static void tile_launch(const uint8_t *qs, const __half *sc, const int8_t *xq,
                        const float *xs, const float *xbs, float *y, float *ssq,
                        int d, int n, int batch, int vec4) {
    auto *kern = k_q40_gemm_tile<RT, EPI>;
    // two stages of 128 rows are 85 / 90 KiB, above the default cap. The
    // attribute belongs to a device: set once on each device the op meets
    // (a step's eager warm-up meets it before any graph capture does)
    static bool set_on[64] = {};
    int device = 0;
    TORCH_CHECK(hipGetDevice(&device) == hipSuccess && device >= 0 && device < 64,
                "tile gemm: no current device");
    if (!set_on[device]) {
        const hipError_t attr = hipFuncSetAttribute(
            reinterpret_cast<const void *>(kern),
            hipFuncAttributeMaxDynamicSharedMemorySize,
            2 * gt_stage_dwords(RT, GT_MAX_ROWS / 16) * 4);
        TORCH_CHECK(attr == hipSuccess, "tile gemm: LDS attribute: ",
                    hipGetErrorString(attr));
        set_on[device] = true;
    }
    const size_t lds = (size_t)2 * gt_stage_dwords(RT, ceil_div(batch, 16)) * 4;
    hipLaunchKernelGGL(kern, dim3(ceil_div(d, RT * 16)), dim3(GT_WAVES * WAVE),
                       lds, cur_stream(), qs, sc, xq, xs, xbs, y, ssq, d, n,
                       batch, vec4);
}

template <int EPI>
static void tile_dispatch(torch::Tensor &qs, torch::Tensor &scales,
                          torch::Tensor &xq, torch::Tensor &xs,
                          torch::Tensor &xbs, torch::Tensor &y, float *ssq,
                          int64_t batch) {
    CHECK_CUDA(qs); CHECK_CONT(qs); CHECK_CONT(scales); CHECK_CONT(xq);
    CHECK_CONT(xs); CHECK_CONT(xbs); CHECK_CUDA(y); CHECK_CONT(y);
    const int d = qs.size(0);
    const int n = qs.size(1) * 2;
    TORCH_CHECK(d >= 1 && n >= QB && n % QB == 0, "n must be a multiple of 32");
    TORCH_CHECK(batch >= 1 && batch <= GT_MAX_ROWS, "tile gemm takes 1..128 rows");
    TORCH_CHECK(xq.size(-1) == n && xq.numel() >= batch * n
                && xs.numel() * QB >= batch * n && xbs.numel() * QB >= batch * n,
                "input triple shorter than [batch, n]");
    TORCH_CHECK(xs.scalar_type() == torch::kFloat32
                && xbs.scalar_type() == torch::kFloat32
                && y.scalar_type() == torch::kFloat32, "xs, xbs and y are f32");
    TORCH_CHECK(y.numel() >= batch * d, "output shorter than [batch, d]");
    const int vec4 = d % 4 == 0
        && reinterpret_cast<uintptr_t>(y.data_ptr<float>()) % 16 == 0;
    auto go = [&](auto launch) {
        launch(qs.data_ptr<uint8_t>(),
               reinterpret_cast<const __half *>(scales.data_ptr<at::Half>()),
               xq.data_ptr<int8_t>(), xs.data_ptr<float>(), xbs.data_ptr<float>(),
               y.data_ptr<float>(), ssq, d, n, (int)batch, vec4);
    };
    if (tile_rt(d) == 1) go(tile_launch<1, EPI>);
    else go(tile_launch<2, EPI>);
}

void q40_gemm_tile(torch::Tensor qs, torch::Tensor scales, torch::Tensor xq,
                   torch::Tensor xs, torch::Tensor xbs, torch::Tensor y,
                   int64_t batch) {
    // y f32 [batch, d] = the Q40 x Q80 product of the first `batch` rows
    tile_dispatch<GT_PLAIN>(qs, scales, xq, xs, xbs, y, nullptr, batch);
}

void q40_gemm_tile_resid(torch::Tensor qs, torch::Tensor scales,
                         torch::Tensor xq, torch::Tensor xs, torch::Tensor xbs,
                         torch::Tensor x, torch::Tensor ssq, int64_t batch) {
    // x[b] += product, the rows' squares into ssq's spread slots
    CHECK_CUDA(ssq); CHECK_CONT(ssq);
    TORCH_CHECK(ssq.scalar_type() == torch::kFloat32
                && ssq.numel() >= batch * SSQ_SPREAD * SSQ_PAD,
                "ssq shorter than `batch` rows of spread slots");
    tile_dispatch<GT_RESID>(qs, scales, xq, xs, xbs, x, ssq.data_ptr<float>(),
                            batch);
}

void register_gemm(py::module &m) {
    m.def("q40_gemm_tile", &q40_gemm_tile, py::arg("qs"), py::arg("scales"),
          py::arg("xq"), py::arg("xs"), py::arg("xbs"), py::arg("y"),
          py::arg("batch"));
    m.def("q40_gemm_tile_resid", &q40_gemm_tile_resid, py::arg("qs"),
          py::arg("scales"), py::arg("xq"), py::arg("xs"), py::arg("xbs"),
          py::arg("x"), py::arg("ssq"), py::arg("batch"));
    m.def("q40_gemm_stream", &q40_gemm_stream, py::arg("qs"), py::arg("scales"),
          py::arg("xq"), py::arg("xs"), py::arg("xbs"), py::arg("y"),
          py::arg("batch"), py::arg("rows") = 0, py::arg("waves") = 0);
    m.def("q40_gemm_stream_resid", &q40_gemm_stream_resid, py::arg("qs"),
          py::arg("scales"), py::arg("xq"), py::arg("xs"), py::arg("xbs"),
          py::arg("x"), py::arg("ssq"), py::arg("batch"), py::arg("rows") = 0,
          py::arg("waves") = 0);
    m.def("q40_gemm_grouped", &q40_gemm_grouped, py::arg("qs"),
          py::arg("scales"), py::arg("xq"), py::arg("xs"), py::arg("plan"),
          py::arg("n_slots"), py::arg("k_slots"), py::arg("y") = py::none(),
          py::arg("oq") = py::none(), py::arg("os") = py::none(),
          py::arg("obs") = py::none(), py::arg("gelu") = false);
    m.def("q40_gemm", &q40_gemm, py::arg("qs"), py::arg("scales"),
          py::arg("xq"), py::arg("xs"), py::arg("y"), py::arg("batch"),
          py::arg("part") = py::none(), py::arg("variant") = -1);
}
