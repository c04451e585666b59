// dllama_amd — Q40xQ80 decode GEMV: plain (with fused epilogues), grouped (MoE) and SwiGLU-fused.

#include "dllama_common.h"

#include <atomic>
#include <mutex>
#include <unordered_map>
#include <vector>

// ------------------------------------------------------------------ Q40 GEMV
// y[b, row] = sum_j w[row, j] * x[b, j]  with W in Q40 planes and x in Q80.
// One wave per output row; lane l streams block l, l+64, ... of the row.
// Weight layout: qs uint8 [d, n/2] (16B per block, byte j = elem j | elem
// j+16 << 4), scales f16 [d, n/32]. Per block:
//   true = sw*sx*(sum_i q_i*x_i - 8*sum_i x_i)  with q in 0..15
// so the nibble unpack is 2 VALU ops per 8 elems and sdot4 does the MAC
// (role of reference matmul_Q80_Q40_F32, nn-cpu-ops.cpp:231-449, and the
//  matmul-forward-q80-q40-f32.comp Vulkan shader).
__device__ __forceinline__ int q40_block_dot(const uint4 wq, const int4 x0,
                                             const int4 x1) {
    const uint32_t wv[4] = {wq.x, wq.y, wq.z, wq.w};
    const int32_t xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    int idot = 0;
    #pragma unroll
    for (int wi = 0; wi < 4; wi++) {
        idot = dot4((int)(wv[wi] & 0x0F0F0F0Fu), xv[wi], idot);            // elems 4wi..4wi+3
        idot = dot4((int)((wv[wi] >> 4) & 0x0F0F0F0Fu), xv[4 + wi], idot); // elems 16+4wi..
    }
    return idot;
}

// The streaming loop of the grouped and SwiGLU kernels: R weight rows
// against one Q80 activation row of n elements (codes xq, block scales xs,
// block sums xbs), into acc[R]. Lane `lane` of `nlanes` takes the block
// pairs lane, lane + nlanes, ...; lane 0 takes the odd trailing block.
// Every accumulator is fed block 2jp, then 2jp + 1, jp ascending, then the
// trailing block, one fmaf each: the integer dots are exact, so this order
// alone fixes the bits of the result. All R rows' weights of a trip are
// loaded ahead of the activations (see RPW at k_q40_gemv). k_q40_gemv runs
// the same loop over NB activation rows and a K slice, in its own body: as
// a call to a function like this one its batch-1 forms came out of hipcc
// with 66 VGPRs in place of 60 (7 waves per SIMD in place of 8), whatever
// the order of the statements here (profiles/r13_gemv_core.md).
template <int R>
__device__ __forceinline__ void q40_q80_rows_dot(
        const uint4 *const (&wrow)[R], const __half *const (&srow)[R],
        const int8_t *xq, const float *xs, const float *xbs, int n,
        int lane, int nlanes, float (&acc)[R]) {
    const int nb = n / QB;
    for (int jp = lane; jp < (nb >> 1); jp += nlanes) {
        const int j = jp << 1;
        uint4 wq0[R], wq1[R];
        float2 sw[R];
        #pragma unroll
        for (int r = 0; r < R; r++) {
            wq0[r] = wrow[r][j];
            wq1[r] = wrow[r][j + 1];
            sw[r] = __half22float2(*reinterpret_cast<const __half2 *>(srow[r] + j));
        }
        const int4 *xrow = reinterpret_cast<const int4 *>(xq) + j * 2;
        const int4 x0 = xrow[0], x1 = xrow[1], x2 = xrow[2], x3 = xrow[3];
        const float2 sx = *reinterpret_cast<const float2 *>(xs + j);
        const float2 bsum = *reinterpret_cast<const float2 *>(xbs + j);
        #pragma unroll
        for (int r = 0; r < R; r++) {
            const int idot0 = q40_block_dot(wq0[r], x0, x1);
            const int idot1 = q40_block_dot(wq1[r], x2, x3);
            acc[r] = fmaf(sw[r].x * sx.x, (float)idot0 - 8.0f * bsum.x, acc[r]);
            acc[r] = fmaf(sw[r].y * sx.y, (float)idot1 - 8.0f * bsum.y, acc[r]);
        }
    }
    if ((nb & 1) && lane == 0) {  // odd trailing block
        const int j = nb - 1;
        const int4 *xb = reinterpret_cast<const int4 *>(xq) + j * 2;
        #pragma unroll
        for (int r = 0; r < R; r++)
            acc[r] = fmaf(__half2float(srow[r][j]) * xs[j],
                          (float)q40_block_dot(wrow[r][j], xb[0], xb[1]) - 8.0f * xbs[j],
                          acc[r]);
    }
}

// the in-kernel MoE gate: every wave recomputes the deterministic top-k from
// the router logits of its batch row and takes entry `want` — removes the
// k_moe_gate launch from the chain. Whole-wave call.
__device__ __forceinline__ int moe_gate_expert(const float *router_row, int n_experts,
                                               int topk, int lane, int want) {
    int gi[16];
    float gw[16];
    moe_gate_wave(router_row, n_experts, topk, lane, gi, gw);
    int e = 0;
    #pragma unroll
    for (int t = 0; t < 16; t++)
        if (t == want) e = gi[t];
    return e;
}

// GEMV epilogue modes: fusing the ops that FOLLOW a matmul into its tail
// removes whole kernels from the per-layer chain (the reference runs each
// as its own op, llm.cpp:263-557).
#define EPI_NONE 0
#define EPI_PACK 4     // TP: plain dot + Q80 WIRE emit (codes then f16 scales,
                       // the all-gather payload) straight from the epilogue
#define EPI_RESID_Q 3  // EPI_RESID + deferred-scale Q80 emit of x*wnorm (one
                       // block per 16-wave wg; consumer applies inv_rms, PRO==2)
#define EPI_RESID_QH 5 // EPI_RESID_Q on 4- or 8-wave wgs: the 16/wpb wgs of a
                       // 32-row block hand their rows to the last arriver,
                       // which emits the block (see the hand-off notes below)
#define EPI_RESID 1  // x[b,row] += v; accumulate sum(x'^2) into 16-way-spread
                     //  slots -> the next norm becomes a single wide pass
#define EPI_ROPE 2   // llama rope: rows (2j,2j+1) are a rotation pair held by
                     //  one RPW=2 wave; q rotated into y, k rotated into the
                     //  KV cache, v copied into the cache

// EPI_RESID_Q assembles the next matmul's Q80 block in workgroup-local LDS,
// so its workgroup must own the block's 32 rows: 16 waves x RPW 2, 128
// workgroups at d = 4096 on 256 CUs. EPI_RESID_QH computes the same values
// on the production shape (4 or 8 waves x RPW 2, 8 or 16 rows per wg) and
// hands the rows over inside the launch: the wg that arrives last at the
// block's ticket quantizes all 32 rows. Each row is folded by one wave with
// the 16-wave form's lane partition and summation order, so x and the Q80
// triple are bit-identical; ssq differs by the order of its float atomics.
// The hand-off has three rules, and the kernel is wrong without any of them:
//  1. sc1 on both sides. x_resid is stored write-through (agent-scope
//     relaxed atomic store = global_store_dwordx2 sc1) and the last arriver
//     reads all 32 rows with agent-scope relaxed atomic loads
//     (global_load_dword sc1), which bypass its CU's L1. That L1 holds the
//     neighbours' OLD values: the wg read its own rows of the same 128-byte
//     lines when it folded the residual. No release/acquire fence is needed,
//     only a wavefront-scope fence to pin the order for the compiler.
//  2. drain before the ticket. Every storing wave runs s_waitcnt vmcnt(0)
//     after its stores, then the wg's barrier, then ONE thread adds to the
//     ticket (agent-scope relaxed fetch_add).
//  3. nobody waits. A wg that is not last exits; no wg polls, spins or
//     sleeps. A launch in which an arrival never comes leaves a stale Q80
//     block; it cannot hang.
// The last arriver stores 0 to the ticket (every arrival has been counted by
// then), so each completed launch leaves the tickets at rest and replays
// need no reset node. Tickets: see resid_q_tickets().
//
// RPW = rows per wave: processing 2 rows per wave doubles the independent
// 16B weight loads in flight per lane (the decode GEMV is HBM-latency
// limited at 1 row/wave). NB = batch columns. PRO = 0: plain Q80 input;
// 2: deferred-scale input, inv_rms from ssq_in applied in the epilogue.
template <int NB, int RPW, int EPI, int PRO>
__global__ void k_q40_gemv(const uint8_t *__restrict__ qs,
                           const __half *__restrict__ scales,
                           const int8_t *__restrict__ xq,
                           const float *__restrict__ xs,
                           const float *__restrict__ xbs,
                           float *__restrict__ y,
                           int d, int n,
                           unsigned long long *__restrict__ amax_scratch,
                           float *__restrict__ x_resid,
                           float *__restrict__ ssq,
                           const float *__restrict__ rope_cache,
                           const int *__restrict__ pos,
                           float *__restrict__ kc,
                           float *__restrict__ vc,
                           int q_dim0, int kv_dim0, int hd,
                           const float *__restrict__ wnorm,
                           const float *__restrict__ ssq_in,
                           float eps, int kv_f16,
                           int8_t *__restrict__ oqq,
                           float *__restrict__ oqs,
                           float *__restrict__ oqbs) {
    const int wpb = blockDim.x / WAVE;
    const int wid = threadIdx.x / WAVE;
    const int row0 = (blockIdx.x * wpb + wid) * RPW;
    const int lane = threadIdx.x % WAVE;
    const int nb = n / QB;
    const int nbp = nb >> 1;
    // K-split (EPI_NONE, B=1 only): gridDim.y slices of the block-pair
    // range; the small-d down-projections underfill the chip at 1 wg per
    // 8 rows, so slicing K multiplies the resident workgroups
    const int nks = gridDim.y;
    const int j0p = (int)((int64_t)nbp * blockIdx.y / nks);
    const int j1p = (int)((int64_t)nbp * (blockIdx.y + 1) / nks);
    const bool wave_valid = row0 < d;
    const int rbase = wave_valid ? row0 : 0;
    [[maybe_unused]] __shared__ float svq[32];  // EPI_RESID_Q block staging

    const uint4 *wrow[RPW];
    const __half *srow[RPW];
    #pragma unroll
    for (int r = 0; r < RPW; r++) {
        const int row = min(rbase + r, d - 1);
        wrow[r] = reinterpret_cast<const uint4 *>(qs + (int64_t)row * (n >> 1));
        srow[r] = scales + (int64_t)row * nb;
    }

    float acc[RPW][NB];
    #pragma unroll
    for (int r = 0; r < RPW; r++)
        #pragma unroll
        for (int b = 0; b < NB; b++) acc[r][b] = 0.0f;

    // EPI_RESID_QH (B=1, RPW=2, d % 32 == 0 so every wave owns two valid
    // rows): lane 0 fetches the wave's residual values ahead of the weight
    // stream, so the fold at the tail does not start with a load from
    // memory. A relaxed atomic load of wavefront scope is an ordinary
    // global_load that hipcc keeps in program order (a plain load is sunk
    // to its use).
    static_assert(EPI != EPI_RESID_QH || (RPW == 2 && NB == 1),
                  "the hand-off epilogue is B=1, RPW=2");
    [[maybe_unused]] float xres[2] = {0.0f, 0.0f};
    if constexpr (EPI == EPI_RESID_QH) {
        if (lane == 0) {
            #pragma unroll
            for (int r = 0; r < 2; r++)
                xres[r] = __hip_atomic_load(&x_resid[rbase + r], __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
    }

    for (int jp = j0p + lane; jp < j1p; jp += WAVE) {
        const int j = jp << 1;
        uint4 wq0[RPW], wq1[RPW];
        float2 sw[RPW];
        #pragma unroll
        for (int r = 0; r < RPW; r++) {
            wq0[r] = wrow[r][j];
            wq1[r] = wrow[r][j + 1];
            sw[r] = __half22float2(*reinterpret_cast<const __half2 *>(srow[r] + j));
        }
        #pragma unroll
        for (int b = 0; b < NB; b++) {
            const int4 *xrow = reinterpret_cast<const int4 *>(xq + (int64_t)b * n) + j * 2;
            const int4 x0 = xrow[0], x1 = xrow[1], x2 = xrow[2], x3 = xrow[3];
            const float2 sx = *reinterpret_cast<const float2 *>(xs + (int64_t)b * nb + j);
            const float2 bsum = *reinterpret_cast<const float2 *>(xbs + (int64_t)b * nb + j);
            #pragma unroll
            for (int r = 0; r < RPW; r++) {
                const int idot0 = q40_block_dot(wq0[r], x0, x1);
                const int idot1 = q40_block_dot(wq1[r], x2, x3);
                acc[r][b] = fmaf(sw[r].x * sx.x, (float)idot0 - 8.0f * bsum.x, acc[r][b]);
                acc[r][b] = fmaf(sw[r].y * sx.y, (float)idot1 - 8.0f * bsum.y, acc[r][b]);
            }
        }
    }
    if ((nb & 1) && lane == 0 && blockIdx.y == nks - 1) {  // odd trailing block
        const int j = nb - 1;
        #pragma unroll
        for (int r = 0; r < RPW; r++) {
            const uint4 wq = wrow[r][j];
            const float sw1 = __half2float(srow[r][j]);
            #pragma unroll
            for (int b = 0; b < NB; b++) {
                const int4 *xb = reinterpret_cast<const int4 *>(xq + (int64_t)b * n) + j * 2;
                const float sx1 = xs[(int64_t)b * nb + j];
                const float bs1 = xbs[(int64_t)b * nb + j];
                const int idot = q40_block_dot(wq, xb[0], xb[1]);
                acc[r][b] = fmaf(sw1 * sx1, (float)idot - 8.0f * bs1, acc[r][b]);
            }
        }
    }

    unsigned long long wave_best = 0ull;
    float ssq_local[NB];
    #pragma unroll
    for (int b = 0; b < NB; b++) ssq_local[b] = 0.0f;
    const int pos0 = (EPI == EPI_ROPE) ? pos[0] : 0;

    #pragma unroll
    for (int b = 0; b < NB; b++) {
        float v[RPW];
        // PRO == 2: the input triple is deferred-scale (see EPI_RESID_Q), so
        // the row's inv_rms is applied here. Computed in the epilogue to
        // keep the ssq load off the kernel's critical start (ahead of the
        // first weight loads)
        float inv = 1.0f;
        if (PRO == 2)
            inv = rsqrtf(ssq_total_wave(ssq_in, b, lane) / n + eps);
        #pragma unroll
        for (int r = 0; r < RPW; r++) {
            v[r] = wave_reduce_sum(acc[r][b]);
            if (PRO == 2) v[r] *= inv;  // deferred inv_rms (scalar/row)
        }
        if (lane != 0 || !wave_valid) continue;
        if (EPI == EPI_ROPE) {
            // RPW==2: rows (rbase, rbase+1) form one llama rotation pair
            const int pb = pos0 + b;
            if (rbase < q_dim0) {
                const int j = (rbase % hd) >> 1;
                const float cr = rope_cache[(int64_t)pb * hd + 2 * j];
                const float ci = rope_cache[(int64_t)pb * hd + 2 * j + 1];
                y[(int64_t)b * d + rbase] = v[0] * cr - v[1 % RPW] * ci;
                y[(int64_t)b * d + rbase + 1] = v[0] * ci + v[1 % RPW] * cr;
            } else if (rbase < q_dim0 + kv_dim0) {
                const int rk = rbase - q_dim0;
                const int j = (rk % hd) >> 1;
                const float cr = rope_cache[(int64_t)pb * hd + 2 * j];
                const float ci = rope_cache[(int64_t)pb * hd + 2 * j + 1];
                const float o0 = v[0] * cr - v[1 % RPW] * ci;
                const float o1 = v[0] * ci + v[1 % RPW] * cr;
                // runtime KV-dtype branch: lane 0 only, once per wave —
                // free next to the weight stream (f16 KV is the default)
                if (kv_f16) {
                    __half *kh = reinterpret_cast<__half *>(kc);
                    kh[(int64_t)pb * kv_dim0 + rk] = __float2half(o0);
                    kh[(int64_t)pb * kv_dim0 + rk + 1] = __float2half(o1);
                } else {
                    kc[(int64_t)pb * kv_dim0 + rk] = o0;
                    kc[(int64_t)pb * kv_dim0 + rk + 1] = o1;
                }
            } else {
                const int rv = rbase - q_dim0 - kv_dim0;
                if (kv_f16) {
                    __half *vh = reinterpret_cast<__half *>(vc);
                    vh[(int64_t)pb * kv_dim0 + rv] = __float2half(v[0]);
                    if (RPW == 2)
                        vh[(int64_t)pb * kv_dim0 + rv + 1] = __float2half(v[1 % RPW]);
                } else {
                    vc[(int64_t)pb * kv_dim0 + rv] = v[0];
                    if (RPW == 2) vc[(int64_t)pb * kv_dim0 + rv + 1] = v[1 % RPW];
                }
            }
        } else if constexpr (EPI == EPI_RESID_QH) {
            // residual fold of the wave's row pair (fetched ahead of the
            // stream), stored write-through (sc1) for the block's last
            // arriver (hand-off rule 1) as ONE 8-byte store. With a load,
            // a wait and a 4-byte store per row the launch was 1.4 us
            // slower: stores count in vmcnt on this target, so the wait for
            // the second row's load also sat out the first store's trip to
            // memory (profiles/r08_resid_q_handoff.md)
            const float xv0 = xres[0] + v[0];
            const float xv1 = xres[1] + v[1 % RPW];
            ssq_local[b] += xv0 * xv0;
            ssq_local[b] += xv1 * xv1;
            const unsigned long long pk = (unsigned long long)__float_as_uint(xv0)
                | ((unsigned long long)__float_as_uint(xv1) << 32);
            __hip_atomic_store(reinterpret_cast<unsigned long long *>(x_resid + rbase),
                               pk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            #pragma unroll
            for (int r = 0; r < RPW; r++) {
                const int row = rbase + r;
                if (row >= d) continue;
                if (EPI == EPI_RESID) {
                    const float xv = x_resid[(int64_t)b * d + row] + v[r];
                    x_resid[(int64_t)b * d + row] = xv;
                    ssq_local[b] += xv * xv;
                } else if (EPI == EPI_RESID_Q) {
                    // residual fold + stage the weighted value for the
                    // wg-local Q80 block (rows of this wg = one block)
                    const float xv = x_resid[(int64_t)b * d + row] + v[r];
                    x_resid[(int64_t)b * d + row] = xv;
                    ssq_local[b] += xv * xv;
                    svq[wid * RPW + r] = xv * wnorm[row];
                } else if (EPI == EPI_PACK) {
                    svq[wid * RPW + r] = v[r];  // partial, packed below
                } else {
                    y[((int64_t)b + (int64_t)blockIdx.y * NB) * d + row] = v[r];
                    if (NB == 1) wave_best = max(wave_best, argmax_pack(v[r], row));
                }
            }
        }
    }
    // amax_scratch has a second tenant: EPI_RESID_QH receives its uint32
    // block tickets in it (see that epilogue). The argmax below must stay
    // EPI_NONE-only so that the two never meet.
    if (EPI == EPI_NONE && NB == 1 && amax_scratch != nullptr) {
        // stage 1 of the greedy argmax: one packed best per workgroup
        __shared__ unsigned long long wb[16];
        if (lane == 0) wb[wid] = wave_best;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long best = wb[0];
            for (int i = 1; i < wpb; i++) best = max(best, wb[i]);
            amax_scratch[blockIdx.x] = best;
        }
    }
    if constexpr (EPI == EPI_PACK) {
        // wire layout (all-gather payload, B=1): int8 codes [d] then f16
        // block scales [d/16 bytes] — what k_sync_quant_pack produces and
        // k_merge_add consumes (no blocksum on the wire)
        __syncthreads();  // publish svq
        if (threadIdx.x < 32 && (int)(blockIdx.x * 32 + threadIdx.x) < d) {
            const Q80Lane c = q80_quant_group32(svq[threadIdx.x]);
            uint8_t *buf = reinterpret_cast<uint8_t *>(oqq);
            buf[blockIdx.x * QB + threadIdx.x] = (uint8_t)(int8_t)c.qf;
            if (threadIdx.x == 0) wire_store_scale(buf, d, blockIdx.x, c.d);
        }
    }
    if constexpr (EPI == EPI_RESID_Q) {
        __shared__ float sredq[16];
        if (lane == 0) sredq[wid] = wave_valid ? ssq_local[0] : 0.0f;
        __syncthreads();  // also publishes svq
        if (threadIdx.x == 0) {
            float t = 0.0f;
            for (int wv = 0; wv < wpb; wv++) t += sredq[wv];
            atomicAdd(ssq_slot(ssq, 0, blockIdx.x), t);
        }
        if (threadIdx.x < 32 && (int)(blockIdx.x * 32 + threadIdx.x) < d) {
            const Q80Lane c = q80_quant_group32(svq[threadIdx.x]);
            oqq[blockIdx.x * QB + threadIdx.x] = (int8_t)c.qf;
            const float bsq = group32_reduce_sum(c.qf);
            if (threadIdx.x == 0) {
                oqs[blockIdx.x] = c.d;
                oqbs[blockIdx.x] = bsq;
            }
        }
    }
    if constexpr (EPI == EPI_RESID_QH) {
        // rule 2: every wave drains its write-through stores, then the barrier
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __shared__ float sredq[8];
        __shared__ unsigned slast;
        if (lane == 0) sredq[wid] = wave_valid ? ssq_local[0] : 0.0f;
        __syncthreads();
        // the tickets ride in the argmax-scratch argument, which this
        // epilogue has no other use for: the kernel's argument list, and
        // with it every other instantiation, stays what it was
        unsigned *tickets = reinterpret_cast<unsigned *>(amax_scratch);
        const unsigned per = 16u / (unsigned)wpb;  // arrivals per 32-row block
        const unsigned blk = blockIdx.x / per;
        if (threadIdx.x == 0) {
            float t = 0.0f;
            for (int wv = 0; wv < wpb; wv++) t += sredq[wv];
            const unsigned prev = __hip_atomic_fetch_add(
                tickets + blk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // behind the ticket: its return is not held up by this one
            atomicAdd(ssq_slot(ssq, 0, blockIdx.x), t);
            const unsigned last = prev == per - 1u;
            if (last)  // all arrivals counted: back to the rest state
                __hip_atomic_store(tickets + blk, 0u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            slast = last;
        }
        __syncthreads();
        if (!slast) return;  // rule 3: not last -> done, nobody waits
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (threadIdx.x < 32 && (int)(blk * 32 + threadIdx.x) < d) {
            const int row = blk * 32 + threadIdx.x;
            const float xv = __hip_atomic_load(&x_resid[row], __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
            const Q80Lane c = q80_quant_group32(xv * wnorm[row]);
            oqq[blk * QB + threadIdx.x] = (int8_t)c.qf;
            const float bsq = group32_reduce_sum(c.qf);
            if (threadIdx.x == 0) {
                oqs[blk] = c.d;
                oqbs[blk] = bsq;
            }
        }
    }
    if (EPI == EPI_RESID) {
        __shared__ float sred[4][NB];
        if (lane == 0)
            #pragma unroll
            for (int b = 0; b < NB; b++) sred[wid][b] = wave_valid ? ssq_local[b] : 0.0f;
        __syncthreads();
        if (threadIdx.x < NB) {
            float t = 0.0f;
            for (int wv = 0; wv < wpb; wv++) t += sred[wv][threadIdx.x];
            atomicAdd(ssq_slot(ssq, threadIdx.x, blockIdx.x), t);
        }
    }
}

// Grouped (MoE) variant: weights [n_experts, d, ...]; slot s uses expert
// expert_idx[s] and input row slot_batch[s]; y [S, d]
// (reference 3-D expert matmul with index indirection, nn-core.hpp:209-213).
// LPP = lanes per 2-row pair. The lane-tiled default (since round 2)
// picks LPP = smallest pow2 >= nbp so every lane stays busy at MoE shapes
// where nbp < 64 (Qwen3-30B w2: nbp=12 left 52 of 64 lanes idle -> the
// ~5x-off-stream round-1 grouped GEMV; see tools/moe_gemv_probe.hip).
// DLLAMA_MOE_V2=0 reverts to the whole-wave (LPP=64) layout.
template <int LPP, bool GATE = false>
__global__ void k_q40_gemv_grouped(const uint8_t *__restrict__ qs,
                                   const __half *__restrict__ scales,
                                   const int8_t *__restrict__ xq,
                                   const float *__restrict__ xs,
                                   const float *__restrict__ xbs,
                                   const int *__restrict__ expert_idx,
                                   float *__restrict__ y,
                                   int d, int n, int k_slots,
                                   const float *__restrict__ router,
                                   int n_experts, int topk,
                                   const float *__restrict__ ssq_in,
                                   float eps) {
    constexpr int NGRP = WAVE / LPP;
    const int wpb = blockDim.x / WAVE;
    const int full_lane = threadIdx.x % WAVE;
    const int grp = full_lane / LPP;
    const int wave_row0 = (blockIdx.x * wpb + threadIdx.x / WAVE) * NGRP * 2;
    const int slot = blockIdx.y;
    if (wave_row0 >= d) return;  // wave-uniform
    // A group past the last row keeps its lanes and streams row 0 unstored:
    // the gate and the ssq total below shuffle across the whole wave, and a
    // shuffle reads 0 from a lane that has exited (with LPP < 64 and d not
    // a multiple of the wave's rows that lost experts and ssq slots).
    const bool valid = wave_row0 + grp * 2 < d;
    const int row0 = valid ? wave_row0 + grp * 2 : 0;
    const int lane = full_lane % LPP;
    const int nb = n / QB;
    int e;
    if constexpr (GATE) {
        const int br = slot / topk;
        e = moe_gate_expert(router + (int64_t)br * n_experts, n_experts, topk,
                            full_lane, slot - br * topk);
    } else {
        e = expert_idx[slot];
    }
    const int b = slot / k_slots;
    const uint4 *wrow[2];
    const __half *srow[2];
    #pragma unroll
    for (int r = 0; r < 2; r++) {
        const int64_t row = (int64_t)e * d + min(row0 + r, d - 1);
        wrow[r] = reinterpret_cast<const uint4 *>(qs + row * (n >> 1));
        srow[r] = scales + row * nb;
    }
    float acc[2] = {};
    q40_q80_rows_dot<2>(wrow, srow, xq + (int64_t)b * n, xs + (int64_t)b * nb,
                        xbs + (int64_t)b * nb, n, lane, LPP, acc);
    float acc0 = acc[0], acc1 = acc[1];
    #pragma unroll
    for (int o = LPP / 2; o > 0; o >>= 1) {
        acc0 += __shfl_down(acc0, o, WAVE);
        acc1 += __shfl_down(acc1, o, WAVE);
    }
    if (ssq_in != nullptr) {
        // deferred-scale input (see EPI_RESID_Q): apply inv_rms per row
        const float inv = rsqrtf(
            ssq_total_wave(ssq_in, b, threadIdx.x % WAVE) / n + eps);
        acc0 *= inv;
        acc1 *= inv;
    }
    if (lane == 0 && valid) {
        y[(int64_t)slot * d + row0] = acc0;
        if (row0 + 1 < d) y[(int64_t)slot * d + row0 + 1] = acc1;
    }
}

// fused W1|W3 GEMV + SwiGLU + Q80 quantize (decode B=1): one kernel replaces
// gemv(w13) + k_swiglu_q80 — per-kernel in-graph overhead is ~3-5 us, so at
// 32 layers/step the saved launch is worth ~150 us/token. The workgroup
// owns one Q80 output block (32 ff indices): wave w computes the W1 and W3
// rows of indices (32*bx+2w, +1) with 4 row streams in flight; the block's
// silu(a)*g values assemble in LDS and the first 32 lanes quantize.
// (reference runs matmul w1, matmul w3, silu, mul, cast as 5 ops,
// llm.cpp:430-448 / nn-cpu-ops.cpp:462-500.)
// GROUPED is the MoE form, with the gate computed in-kernel from the router
// logits: for decode (B=1) this single launch replaces moe_gate + grouped
// w13 GEMV + swiglu_q80 (reference runs repeat_z, gate matmul, softmax,
// moe_gate, grouped w1/w3, silu, mul, cast — llm.cpp:450-487). Weights
// [E, 2*ff, n/2], workgroup = one Q80 block of expert slot blockIdx.y's
// output, oq/os/obs [n_slots, ff]. The dense form is expert 0, x row 0,
// slot 0.
template <bool GELU, bool GROUPED>
__global__ __launch_bounds__(1024) void k_q40_gemv_swiglu(
        const uint8_t *__restrict__ qs, const __half *__restrict__ scales,
        const int8_t *__restrict__ xq, const float *__restrict__ xs,
        const float *__restrict__ xbs, int ff, int n,
        const float *__restrict__ router, int n_experts, int topk,
        int8_t *__restrict__ oq, float *__restrict__ os,
        float *__restrict__ obs) {
    const int wave = threadIdx.x / WAVE;  // 16 waves, 2 ff indices each
    const int lane = threadIdx.x % WAVE;
    int slot = 0, br = 0, e = 0;
    if constexpr (GROUPED) {
        slot = blockIdx.y;
        br = slot / topk;
        e = moe_gate_expert(router + (int64_t)br * n_experts, n_experts, topk,
                            lane, slot - br * topk);
    }
    const int i0 = blockIdx.x * 32 + 2 * wave;
    const int nb = n / QB;
    const int rows[4] = {i0, i0 + 1, ff + i0, ff + i0 + 1};
    const uint4 *wrow[4];
    const __half *srow[4];
    #pragma unroll
    for (int r = 0; r < 4; r++) {
        const int64_t row = (int64_t)e * 2 * ff + rows[r];
        wrow[r] = reinterpret_cast<const uint4 *>(qs + row * (n >> 1));
        srow[r] = scales + row * nb;
    }
    float acc[4] = {};
    q40_q80_rows_dot<4>(wrow, srow, xq + (int64_t)br * n, xs + (int64_t)br * nb,
                        xbs + (int64_t)br * nb, n, lane, WAVE, acc);
    #pragma unroll
    for (int r = 0; r < 4; r++) acc[r] = wave_reduce_sum(acc[r]);
    __shared__ float sv[32];
    if (lane == 0) {
        #pragma unroll
        for (int t = 0; t < 2; t++) {
            const float av = acc[t], gv = acc[2 + t];
            const float act = GELU
                ? 0.5f * av * (1.0f + tanhf(0.797884560802865f * (av + 0.044715f * av * av * av)))
                : av / (1.0f + __expf(-av));
            sv[2 * wave + t] = act * gv;
        }
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        // ff % 32 == 0 (checked by the bindings), so a slot's ff codes are
        // ff / QB whole blocks: code index slot * ff + bx * QB = blk * QB
        const int64_t blk = (int64_t)slot * (ff / QB) + blockIdx.x;
        const Q80Lane c = q80_quant_group32(sv[threadIdx.x]);
        oq[blk * QB + threadIdx.x] = (int8_t)c.qf;
        const float bsum = group32_reduce_sum(c.qf);
        if (threadIdx.x == 0) { os[blk] = c.d; obs[blk] = bsum; }
    }
}

// K-split completion for the deferred down-projections: x += sum of the
// K-slices' partials, ssq, and the DEFERRED Q80 emit of x*wnorm — the
// same epilogue EPI_RESID_Q provides, but fed by a fully-filled K-split
// GEMV instead of a 1-wg-per-32-rows underfilled one. 256-elem wgs.
__global__ void k_add_ssq_q(float *__restrict__ x,
                            const float *__restrict__ parts,
                            float *__restrict__ ssq,
                            const float *__restrict__ wnorm,
                            int8_t *__restrict__ oq,
                            float *__restrict__ os,
                            float *__restrict__ obs,
                            int n, int nks) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    float acc = x[i];
    for (int k = 0; k < nks; k++)
        acc += parts[(int64_t)k * n + i];
    x[i] = acc;
    ssq_block_add<4>(ssq, 0, acc * acc);
    const Q80Lane c = q80_quant_group32(acc * wnorm[i]);
    oq[i] = (int8_t)c.qf;
    const float bsum = group32_reduce_sum(c.qf);
    if ((threadIdx.x & 31) == 0) {
        os[i / QB] = c.d;
        obs[i / QB] = bsum;
    }
}

// ============================================================== host bindings

struct GemvEpi {
    unsigned long long *slot = nullptr;
    float *x_resid = nullptr;
    float *ssq = nullptr;
    const float *cache = nullptr;
    const int *pos = nullptr;
    float *kc = nullptr;  // f32 or f16 rows; kv_f16 says which
    float *vc = nullptr;
    int q_dim0 = 0, kv_dim0 = 0, hd = 0;
    int kv_f16 = 0;
    bool force_rpw2 = false;
    int ksplit = 1;  // gridDim.y K slices (EPI_NONE, batch 1): y is [ksplit, d]
    // PRO=2 (deferred-scale input): the row ssq and eps for inv_rms
    const float *ssq_in = nullptr;
    float eps = 0.0f;
    // EPI_RESID_Q deferred-quant: norm weight in, Q80 triple out
    // (EPI_PACK: oqq is the wire row)
    const float *wnorm = nullptr;
    int8_t *oqq = nullptr;
    float *oqs = nullptr;
    float *oqbs = nullptr;
    // EPI_RESID_QH: waves per workgroup (4 or 8); its block tickets travel
    // in `slot`
    int waves = 0;
};

// rows per wave of the batch-1 GEMV over d rows: RPW=2 halves the wave count
// for 2x per-lane loads in flight; tunable crossover (DLLAMA_RPW1_MAX).
// The launch grid and the argmax scratch count both follow from it.
static int gemv_rpw1(int64_t d, bool force_rpw2) {
    static const int rpw1_max =
        std::getenv("DLLAMA_RPW1_MAX") ? atoi(std::getenv("DLLAMA_RPW1_MAX")) : 0;
    return (force_rpw2 || (d >= 2048 && d > rpw1_max)) ? 2 : 1;
}

template <int EPI, int PRO>
static void gemv_launch(torch::Tensor &qs, torch::Tensor &scales, torch::Tensor &xq,
                        torch::Tensor &xs, torch::Tensor &xbs, float *y,
                        int64_t batch, const GemvEpi &e) {
    const int d = qs.size(0);
    const int n = qs.size(1) * 2;
    TORCH_CHECK(xq.size(-1) == n, "x width mismatch");
    TORCH_CHECK(n % QB == 0, "n must be a multiple of 32");
    // EPI_RESID_Q / EPI_PACK: 16 waves x RPW2 = 32 rows per wg = one block;
    // EPI_RESID_QH: 4 or 8 waves, chosen by the caller (resid_q_waves)
    const int waves_per_block = (EPI == EPI_RESID_QH) ? e.waves
        : (EPI == EPI_RESID_Q || EPI == EPI_PACK) ? 16 : 4;
    const dim3 block(waves_per_block * WAVE);
    auto launch = [&](auto nb_const, auto rpw_const) {
        constexpr int RPW = decltype(rpw_const)::value;
        const dim3 grid(ceil_div(d, waves_per_block * RPW), e.ksplit);
        hipLaunchKernelGGL((k_q40_gemv<decltype(nb_const)::value, RPW, EPI, PRO>), grid,
                           block, 0, cur_stream(),
                           qs.data_ptr<uint8_t>(),
                           reinterpret_cast<const __half *>(scales.data_ptr<at::Half>()),
                           xq.data_ptr<int8_t>(), xs.data_ptr<float>(),
                           xbs.data_ptr<float>(), y, d, n,
                           e.slot, e.x_resid, e.ssq,
                           e.cache, e.pos, e.kc, e.vc, e.q_dim0, e.kv_dim0, e.hd,
                           e.wnorm, e.ssq_in, e.eps, e.kv_f16,
                           e.oqq, e.oqs, e.oqbs);
    };
    std::integral_constant<int, 1> r1;
    std::integral_constant<int, 2> r2;
    // RPW per batch size. Rotation pairs (EPI_ROPE) need RPW=2 at every
    // batch; otherwise decode batches 2/4 take 2, prefill batches 1, and
    // batch 1 asks gemv_rpw1. `if constexpr` so only the (NB, RPW) pairs
    // this selection can reach are instantiated — a plain `if` would keep
    // dead RPW combinations (that additionally spill) alive
    auto launch_nb = [&](auto nb_const) {
        constexpr int NB = decltype(nb_const)::value;
        if constexpr (EPI == EPI_RESID_QH) {
            // B=1, RPW=2 only: the row-pair fold and the block/ticket
            // arithmetic assume it
            if constexpr (NB == 1) launch(nb_const, r2);
            else TORCH_CHECK(false, "resid_q hand-off form is batch 1 only");
        } else if constexpr (EPI == EPI_ROPE || NB == 2 || NB == 4) {
            launch(nb_const, r2);
        } else if constexpr (NB > 4) {
            launch(nb_const, r1);
        } else {
            if (gemv_rpw1(d, e.force_rpw2) == 2) launch(nb_const, r2);
            else launch(nb_const, r1);
        }
    };
    switch (batch) {
        case 1: launch_nb(std::integral_constant<int, 1>{}); break;
        case 2: launch_nb(std::integral_constant<int, 2>{}); break;
        case 4: launch_nb(std::integral_constant<int, 4>{}); break;
        case 8:
        case 16:
        case 32:
            // PRO (deferred inv_rms) is a batch<=4 decode path
            if constexpr (PRO) {
                TORCH_CHECK(false, "fused-norm GEMV supports batch <= 4");
            } else {
                if (batch == 8) launch_nb(std::integral_constant<int, 8>{});
                else if (batch == 16) launch_nb(std::integral_constant<int, 16>{});
                else launch_nb(std::integral_constant<int, 32>{});
            }
            break;
        default: TORCH_CHECK(false, "unsupported batch ", batch);
    }
}

void q40_gemv(torch::Tensor qs, torch::Tensor scales, torch::Tensor xq,
              torch::Tensor xs, torch::Tensor xbs, torch::Tensor y, int64_t batch,
              c10::optional<torch::Tensor> amax_slot = c10::nullopt,
              c10::optional<torch::Tensor> ssq_in = c10::nullopt,
              double eps = 0.0) {
    // ssq_in given: the xq triple is DEFERRED (scales exclude inv_rms, see
    // EPI_RESID_Q); the kernel applies inv = rsqrt(ssq/n + eps) per row
    CHECK_CUDA(qs); CHECK_CONT(qs); CHECK_CONT(xq);
    GemvEpi e;
    if (amax_slot.has_value())
        e.slot = reinterpret_cast<unsigned long long *>(amax_slot->data_ptr<int64_t>());
    if (ssq_in.has_value()) {
        e.ssq_in = ssq_in->data_ptr<float>();
        e.eps = (float)eps;
        gemv_launch<EPI_NONE, 2>(qs, scales, xq, xs, xbs, y.data_ptr<float>(), batch, e);
    } else {
        gemv_launch<EPI_NONE, 0>(qs, scales, xq, xs, xbs, y.data_ptr<float>(), batch, e);
    }
}

void q40_gemv_pack(torch::Tensor qs, torch::Tensor scales, torch::Tensor xq,
                   torch::Tensor xs, torch::Tensor xbs, torch::Tensor wire) {
    // TP down-projection: plain partial dot + Q80 WIRE emit in one launch
    // (replaces gemv-into-partial + sync_quant_pack). B=1 decode only.
    CHECK_CUDA(qs); CHECK_CONT(qs); CHECK_CONT(xq);
    const int d = qs.size(0);
    TORCH_CHECK(d % 32 == 0, "gemv_pack needs d % 32 == 0");
    GemvEpi e;
    e.oqq = reinterpret_cast<int8_t *>(wire.data_ptr<uint8_t>());
    e.force_rpw2 = true;
    gemv_launch<EPI_PACK, 0>(qs, scales, xq, xs, xbs, nullptr, 1, e);
}

void q40_gemv_ksplit(torch::Tensor qs, torch::Tensor scales, torch::Tensor xq,
                     torch::Tensor xs, torch::Tensor xbs, torch::Tensor part,
                     int64_t ks) {
    // B=1 K-split GEMV into part[ks, d] (see k_add_ssq_q for the merge)
    CHECK_CUDA(qs); CHECK_CONT(qs); CHECK_CONT(xq);
    TORCH_CHECK((int64_t)ks * qs.size(0) <= part.numel(), "part buffer too small");
    GemvEpi e;
    e.force_rpw2 = true;  // 8 rows per 4-wave wg at every d
    e.ksplit = (int)ks;
    gemv_launch<EPI_NONE, 0>(qs, scales, xq, xs, xbs, part.data_ptr<float>(), 1, e);
}

void add_ssq_q(torch::Tensor x, torch::Tensor parts, torch::Tensor ssq,
               torch::Tensor wnorm, torch::Tensor oq, torch::Tensor os,
               torch::Tensor obs, int64_t nks) {
    CHECK_CUDA(x);
    const int n = x.size(-1);
    TORCH_CHECK(n % 256 == 0, "add_ssq_q needs dim % 256 == 0");
    hipLaunchKernelGGL(k_add_ssq_q, dim3(n / 256), dim3(256), 0, cur_stream(),
                       x.data_ptr<float>(), parts.data_ptr<float>(),
                       ssq.data_ptr<float>(), wnorm.data_ptr<float>(),
                       oq.data_ptr<int8_t>(), os.data_ptr<float>(),
                       obs.data_ptr<float>(), n, (int)nks);
}

// waves per workgroup of the resid_q down-projection over a [d, n] matrix:
// 16 = one block per wg (EPI_RESID_Q), 4 / 8 = the hand-off form
// (EPI_RESID_QH) with four / two arrivals per block. DLLAMA_RESID_Q_WAVES
// (4, 8 or 16, read once) forces one form for A/B runs and the equality
// test; q40_gemv_resid_q_waves() does the same from inside a process.
// Default rule, from the isolated out-of-cache timings of
// `tools/kernel_bench.py resid` (profiles/r08_resid_q_handoff.md): the
// hand-off's tail costs more than the fuller chip gives back unless a row is
// long. 8 waves won at every measured shape with n >= 8192 and d < 8192
// (8B w2 12.8 -> 10.3 us, 1B/3B w2 -0.3..-0.5 us) and beat 4 waves there;
// 16 waves won at every n <= 4096 (by 0.5..0.8 us) and at d = 8192.
// q40_gemv_resid_q_waves() is process-global and meant for the tests and
// tools/kernel_bench.py only: whoever sets it puts it back to 0.
static std::atomic<int> g_resid_q_waves_override{0};

static int resid_q_waves(int d, int n) {
    static const int env_waves =
        std::getenv("DLLAMA_RESID_Q_WAVES") ? atoi(std::getenv("DLLAMA_RESID_Q_WAVES")) : 0;
    const int ov = g_resid_q_waves_override.load();
    const int forced = ov ? ov : env_waves;
    if (forced == 4 || forced == 8 || forced == 16) return forced;
    return (d < 8192 && n >= 8192) ? 8 : 16;
}

void q40_gemv_resid_q_waves(int64_t waves) {
    TORCH_CHECK(waves == 0 || waves == 4 || waves == 8 || waves == 16,
                "resid_q waves: 0 (default rule), 4, 8 or 16");
    g_resid_q_waves_override.store((int)waves);
}

// EPI_RESID_QH tickets: one uint32 per 32-row block, at rest 0. Owned here
// and keyed by the residual buffer's address: two launches that may be in
// flight at once never share x, so they never share tickets, and the
// binding needs no new argument. An array is allocated and zeroed at the
// first launch on its x, which must be outside stream capture (every
// capture in this project follows eager warm-ups of the same calls); a
// captured graph then names memory that is never freed: entries are kept
// for the life of the process (4 bytes per block per distinct x address;
// a reused address finds its old tickets, at rest).
static unsigned *resid_q_tickets(const torch::Tensor &x, int nblocks) {
    static std::mutex mu;
    // leaked on purpose: no device free during static destruction
    static auto *store = new std::unordered_map<const void *, torch::Tensor>();
    static auto *outgrown = new std::vector<torch::Tensor>();
    std::lock_guard<std::mutex> lock(mu);
    const void *key = x.data_ptr();
    auto it = store->find(key);
    if (it != store->end() && it->second.numel() >= nblocks)
        return reinterpret_cast<unsigned *>(it->second.data_ptr<int32_t>());
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    C10_HIP_CHECK(hipStreamIsCapturing(cur_stream(), &st));
    TORCH_CHECK(st == hipStreamCaptureStatusNone,
                "q40_gemv_resid_q: first use of this residual buffer (or with "
                "a larger d) inside stream capture; run the call eagerly once "
                "before capturing so its block tickets exist");
    torch::Tensor t = torch::zeros({nblocks}, x.options().dtype(torch::kInt32));
    // zeroed on this stream; make it hold for a later launch on any stream
    C10_HIP_CHECK(hipStreamSynchronize(cur_stream()));
    if (it != store->end()) {
        outgrown->push_back(it->second);  // a graph may still name it
        it->second = t;
    } else {
        store->emplace(key, t);
    }
    return reinterpret_cast<unsigned *>(t.data_ptr<int32_t>());
}

void q40_gemv_resid_q(torch::Tensor qs, torch::Tensor scales, torch::Tensor xq,
                      torch::Tensor xs, torch::Tensor xbs, torch::Tensor x,
                      torch::Tensor ssq, torch::Tensor wnorm, torch::Tensor oq,
                      torch::Tensor os, torch::Tensor obs) {
    // decode down-projection with fused residual + ssq + DEFERRED Q80 emit
    // of x*wnorm: replaces gemv_resid + norm_quant (the consumer runs with
    // ssq_in to apply inv_rms). B=1 only; 16-wave wgs (one block per wg) or
    // the 4/8-wave hand-off form, see resid_q_waves().
    CHECK_CUDA(qs); CHECK_CONT(qs); CHECK_CONT(xq);
    const int d = qs.size(0);
    TORCH_CHECK(d % 32 == 0, "resid_q needs d % 32 == 0");
    TORCH_CHECK(x.numel() >= d && wnorm.numel() >= d && oq.numel() >= d,
                "resid_q: x, wnorm and oq need d elements");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr<float>()) % 8 == 0,
                "resid_q: x must be 8-byte aligned (row pairs are stored whole)");
    GemvEpi e;
    e.x_resid = x.data_ptr<float>();
    e.ssq = ssq.data_ptr<float>();
    e.wnorm = wnorm.data_ptr<float>();
    e.oqq = oq.data_ptr<int8_t>();
    e.oqs = os.data_ptr<float>();
    e.oqbs = obs.data_ptr<float>();
    e.force_rpw2 = true;
    const int waves = resid_q_waves(d, (int)qs.size(1) * 2);
    if (waves == 16) {
        gemv_launch<EPI_RESID_Q, 0>(qs, scales, xq, xs, xbs, x.data_ptr<float>(), 1, e);
    } else {
        e.waves = waves;
        e.slot = reinterpret_cast<unsigned long long *>(resid_q_tickets(x, d / 32));
        gemv_launch<EPI_RESID_QH, 0>(qs, scales, xq, xs, xbs, x.data_ptr<float>(), 1, e);
    }
}

void q40_gemv_resid(torch::Tensor qs, torch::Tensor scales, torch::Tensor xq,
                    torch::Tensor xs, torch::Tensor xbs, torch::Tensor x,
                    torch::Tensor ssq, int64_t batch) {
    CHECK_CUDA(qs); CHECK_CONT(qs); CHECK_CONT(xq);
    TORCH_CHECK(batch <= 32, "RESID epilogue LDS sized for batch<=32");
    GemvEpi e;
    e.x_resid = x.data_ptr<float>();
    e.ssq = ssq.data_ptr<float>();
    gemv_launch<EPI_RESID, 0>(qs, scales, xq, xs, xbs, x.data_ptr<float>(), batch, e);
}

void q40_gemv_rope(torch::Tensor qs, torch::Tensor scales, torch::Tensor xq,
                   torch::Tensor xs, torch::Tensor xbs, torch::Tensor y,
                   int64_t batch, torch::Tensor cache, torch::Tensor pos,
                   torch::Tensor kc, torch::Tensor vc, int64_t q_dim0,
                   int64_t kv_dim0, int64_t head_dim,
                   c10::optional<torch::Tensor> ssq_in = c10::nullopt,
                   double eps = 0.0) {
    CHECK_CUDA(qs); CHECK_CONT(qs); CHECK_CONT(xq);
    // the epilogue holds two rows per wave and cannot see a Q80 block
    TORCH_CHECK(kc.scalar_type() != at::kChar && vc.scalar_type() != at::kChar,
                "q40_gemv_rope has no Q80 KV cache form: run the QKV GEMV "
                "and rope_kv(..., k_scales=, v_scales=)");
    GemvEpi e;
    e.cache = cache.data_ptr<float>();
    e.pos = pos.data_ptr<int>();
    e.kv_f16 = kc.scalar_type() == at::kHalf ? 1 : 0;
    e.kc = static_cast<float *>(kc.data_ptr());
    e.vc = static_cast<float *>(vc.data_ptr());
    e.q_dim0 = (int)q_dim0;
    e.kv_dim0 = (int)kv_dim0;
    e.hd = (int)head_dim;
    e.force_rpw2 = true;  // rotation pairs live in one RPW=2 wave
    if (ssq_in.has_value()) {  // deferred-scale input (see q40_gemv)
        e.ssq_in = ssq_in->data_ptr<float>();
        e.eps = (float)eps;
        gemv_launch<EPI_ROPE, 2>(qs, scales, xq, xs, xbs, y.data_ptr<float>(), batch, e);
    } else {
        gemv_launch<EPI_ROPE, 0>(qs, scales, xq, xs, xbs, y.data_ptr<float>(), batch, e);
    }
}

int64_t q40_gemv_argmax_blocks(int64_t d) {
    // stage-1 argmax scratch entries for a batch-1 GEMV over d rows: one
    // per 4-wave workgroup of the plain q40_gemv launch
    return ceil_div(d, 4 * gemv_rpw1(d, false));
}

void q40_gemv_grouped(torch::Tensor qs, torch::Tensor scales, torch::Tensor xq,
                      torch::Tensor xs, torch::Tensor xbs, torch::Tensor expert_idx,
                      torch::Tensor y, int64_t k_slots, int64_t variant = -1,
                      c10::optional<torch::Tensor> router = c10::nullopt,
                      int64_t topk = 0, int64_t n_slots_override = 0,
                      c10::optional<torch::Tensor> ssq_in = c10::nullopt,
                      double eps = 0.0) {
    // router given: expert ids come from the in-kernel gate over the router
    // logits [B, n_experts] (expert_idx is then ignored); n_slots_override
    // sets the slot count (it can no longer come from expert_idx.numel())
    CHECK_CUDA(qs); CHECK_CONT(qs);
    const int d = qs.size(1);
    const int n = qs.size(2) * 2;
    const int n_slots = n_slots_override > 0 ? (int)n_slots_override
                                             : (int)expert_idx.numel();
    const int waves_per_block = 4;
    // lane-tiled (v2) default since round 2 (validated: 1.4-1.8x at
    // Qwen3-30B shapes); DLLAMA_MOE_V2=0 reverts to the 64-lane layout
    static const bool env_v2 = !std::getenv("DLLAMA_MOE_V2")
        || atoi(std::getenv("DLLAMA_MOE_V2")) != 0;
    // v2: LPP = smallest power of two >= nbp (clamped [8, 64]) so every
    // lane has work; rows per wave scale up by 64/LPP
    int lpp = 64;
    if (variant < 0 ? env_v2 : variant == 1) {
        const int nbp = (n / QB) >> 1;
        lpp = 8;
        while (lpp < nbp && lpp < 64) lpp <<= 1;
    }
    const int rows_per_wg = waves_per_block * 2 * (WAVE / lpp);
    const dim3 grid(ceil_div(d, rows_per_wg), n_slots);
    const dim3 block(waves_per_block * WAVE);
    const bool gate = router.has_value();
    const float *rp = gate ? router->data_ptr<float>() : nullptr;
    const int ne = gate ? (int)router->size(-1) : 0;
    const float *sqp = ssq_in.has_value() ? ssq_in->data_ptr<float>() : nullptr;
    auto launch = [&](auto k) {
        hipLaunchKernelGGL(k, grid, block, 0, cur_stream(),
                           qs.data_ptr<uint8_t>(),
                           reinterpret_cast<const __half *>(scales.data_ptr<at::Half>()),
                           xq.data_ptr<int8_t>(), xs.data_ptr<float>(),
                           xbs.data_ptr<float>(), expert_idx.data_ptr<int>(),
                           y.data_ptr<float>(), d, n, (int)k_slots,
                           rp, ne, (int)topk, sqp, (float)eps);
    };
    if (gate) {
        switch (lpp) {
            case 8: launch(k_q40_gemv_grouped<8, true>); break;
            case 16: launch(k_q40_gemv_grouped<16, true>); break;
            case 32: launch(k_q40_gemv_grouped<32, true>); break;
            default: launch(k_q40_gemv_grouped<64, true>); break;
        }
    } else {
        switch (lpp) {
            case 8: launch(k_q40_gemv_grouped<8>); break;
            case 16: launch(k_q40_gemv_grouped<16>); break;
            case 32: launch(k_q40_gemv_grouped<32>); break;
            default: launch(k_q40_gemv_grouped<64>); break;
        }
    }
}

// one launch of k_q40_gemv_swiglu over `n_slots` expert slots of ff/32
// blocks each; router == nullptr is the dense form
static void swiglu_launch(torch::Tensor &qs, torch::Tensor &scales, torch::Tensor &xq,
                          torch::Tensor &xs, torch::Tensor &xbs, int ff, int n,
                          int64_t n_slots, const float *router, int n_experts,
                          int64_t topk, torch::Tensor &oq, torch::Tensor &os,
                          torch::Tensor &obs, bool gelu) {
    TORCH_CHECK(ff % 32 == 0, "fused swiglu GEMV needs ff % 32 == 0");
    TORCH_CHECK(xq.size(-1) == n, "x width mismatch");
    auto launch = [&](auto k) {
        hipLaunchKernelGGL(k, dim3(ff / 32, n_slots), dim3(16 * WAVE), 0, cur_stream(),
                           qs.data_ptr<uint8_t>(),
                           reinterpret_cast<const __half *>(scales.data_ptr<at::Half>()),
                           xq.data_ptr<int8_t>(), xs.data_ptr<float>(),
                           xbs.data_ptr<float>(), ff, n, router, n_experts,
                           (int)topk, oq.data_ptr<int8_t>(), os.data_ptr<float>(),
                           obs.data_ptr<float>());
    };
    if (router == nullptr) {
        if (gelu) launch(k_q40_gemv_swiglu<true, false>);
        else launch(k_q40_gemv_swiglu<false, false>);
    } else {
        if (gelu) launch(k_q40_gemv_swiglu<true, true>);
        else launch(k_q40_gemv_swiglu<false, true>);
    }
}

void q40_gemv_swiglu(torch::Tensor qs, torch::Tensor scales, torch::Tensor xq,
                     torch::Tensor xs, torch::Tensor xbs, torch::Tensor oq,
                     torch::Tensor os, torch::Tensor obs, bool gelu = false) {
    // B=1 decode FFN: W1|W3 GEMV + SwiGLU + Q80 emit, one launch
    CHECK_CUDA(qs); CHECK_CONT(qs); CHECK_CONT(xq);
    swiglu_launch(qs, scales, xq, xs, xbs, (int)qs.size(0) / 2, (int)qs.size(1) * 2,
                  1, nullptr, 0, 0, oq, os, obs, gelu);
}

void q40_gemv_grouped_swiglu(torch::Tensor qs, torch::Tensor scales,
                             torch::Tensor xq, torch::Tensor xs,
                             torch::Tensor xbs, torch::Tensor oq,
                             torch::Tensor os, torch::Tensor obs,
                             int64_t n_slots, torch::Tensor router,
                             int64_t topk, bool gelu = false) {
    // decode MoE FFN up-projection: gate + grouped W1|W3 GEMV + SwiGLU +
    // Q80 emit in one launch. qs [E, 2*ff, n/2]; oq/os/obs are the
    // [n_slots, ff] Q80 triple.
    CHECK_CUDA(qs); CHECK_CONT(qs); CHECK_CONT(xq);
    const int ff = (int)qs.size(1) / 2;
    TORCH_CHECK(ff % 32 == 0, "fused grouped swiglu needs ff % 32 == 0");
    swiglu_launch(qs, scales, xq, xs, xbs, ff, (int)qs.size(2) * 2, n_slots,
                  router.data_ptr<float>(), (int)router.size(-1), topk,
                  oq, os, obs, gelu);
}

void register_gemv(py::module &m) {
    m.def("q40_gemv", &q40_gemv, py::arg("qs"), py::arg("scales"), py::arg("xq"),
          py::arg("xs"), py::arg("xbs"), py::arg("y"), py::arg("batch"),
          py::arg("amax_slot") = py::none(), py::arg("ssq_in") = py::none(),
          py::arg("eps") = 0.0);
    m.def("q40_gemv_resid", &q40_gemv_resid);
    m.def("q40_gemv_resid_q", &q40_gemv_resid_q);
    m.def("q40_gemv_resid_q_waves", &q40_gemv_resid_q_waves);
    m.def("q40_gemv_pack", &q40_gemv_pack);
    m.def("q40_gemv_ksplit", &q40_gemv_ksplit);
    m.def("add_ssq_q", &add_ssq_q);
    m.def("q40_gemv_rope", &q40_gemv_rope, py::arg("qs"), py::arg("scales"),
          py::arg("xq"), py::arg("xs"), py::arg("xbs"), py::arg("y"),
          py::arg("batch"), py::arg("cache"), py::arg("pos"), py::arg("kc"),
          py::arg("vc"), py::arg("q_dim0"), py::arg("kv_dim0"),
          py::arg("head_dim"), py::arg("ssq_in") = py::none(),
          py::arg("eps") = 0.0);
    m.def("q40_gemv_swiglu", &q40_gemv_swiglu, py::arg("qs"), py::arg("scales"),
          py::arg("xq"), py::arg("xs"), py::arg("xbs"), py::arg("oq"),
          py::arg("os"), py::arg("obs"), py::arg("gelu") = false);
    m.def("q40_gemv_grouped", &q40_gemv_grouped, py::arg("qs"),
          py::arg("scales"), py::arg("xq"), py::arg("xs"), py::arg("xbs"),
          py::arg("expert_idx"), py::arg("y"), py::arg("k_slots"),
          py::arg("variant") = -1, py::arg("router") = py::none(),
          py::arg("topk") = 0, py::arg("n_slots") = 0,
          py::arg("ssq_in") = py::none(), py::arg("eps") = 0.0);
    m.def("q40_gemv_grouped_swiglu", &q40_gemv_grouped_swiglu, py::arg("qs"),
          py::arg("scales"), py::arg("xq"), py::arg("xs"), py::arg("xbs"),
          py::arg("oq"), py::arg("os"), py::arg("obs"), py::arg("n_slots"),
          py::arg("router"), py::arg("topk"), py::arg("gelu") = false);
    m.def("q40_gemv_argmax_blocks", &q40_gemv_argmax_blocks);
}
