// dllama_amd — hand-written CDNA4 (gfx950) kernels for Q40xQ80 LLM inference.
//
// Design notes (MI355X-first, not a port):
//  - decode is HBM-bandwidth bound on the Q40 weight stream; the GEMV keeps
//    one wave per output row streaming 16B nibble payloads per lane and does
//    the int8 math with v_dot4 (sdot4), correcting the Q40 "-8" offset with
//    precomputed per-block activation sums (so nibbles never get unpacked
//    to signed values).
//  - every runtime scalar the decode loop needs (position) is read from
//    device memory so whole-token hipGraph capture works.
//  - role parity with the reference op set: src/nn/nn-cpu-ops.cpp and the
//    Vulkan shaders in src/nn/vulkan/ (see SURVEY.md §2.3/§2.5).
//
// All f32 accumulation (parity with the reference numerics).
//
// This header is what the per-family sources share: constants, reductions,
// the Q80 / wire / ssq-slot idioms, host-side checks and the register_*
// prototypes. Kernels, their launchers and their bindings live in
//   quant_norm.hip  gemv.hip  gemm.hip  attn.hip  moe.hip  sync.hip
//   sampler.hip  logprob.hip
// host-only code (CPU matmul, BPE encoder) in host.hip, the module in
// module.hip.

#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <torch/extension.h>
#include <cstdlib>
#include <ATen/hip/HIPContext.h>

#define WAVE 64
#define QB 32  // quant block size
#define SSQ_SPREAD 16
#define SSQ_PAD 32  // floats between spread slots (own 128B cacheline)

static inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

#if __has_builtin(__builtin_amdgcn_sdot4)
__device__ __forceinline__ int dot4(int a, int b, int c) {
    return __builtin_amdgcn_sdot4(a, b, c, false);
}
#else
__device__ __forceinline__ int dot4(int a, int b, int c) {
    const char4 va = *reinterpret_cast<const char4 *>(&a);
    const char4 vb = *reinterpret_cast<const char4 *>(&b);
    return c + va.x * vb.x + va.y * vb.y + va.z * vb.z + va.w * vb.w;
}
#endif

__device__ __forceinline__ float wave_reduce_sum(float v) {
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off, WAVE);
    return v;
}

__device__ __forceinline__ float group32_reduce_max(float v) {
    #pragma unroll
    for (int off = 16; off > 0; off >>= 1)
        v = fmaxf(v, __shfl_xor(v, off, 32));
    return v;
}

__device__ __forceinline__ float group32_reduce_sum(float v) {
    #pragma unroll
    for (int off = 16; off > 0; off >>= 1)
        v += __shfl_xor(v, off, 32);
    return v;
}

__device__ __forceinline__ float group16_reduce_sum(float v) {
    #pragma unroll
    for (int off = 8; off > 0; off >>= 1)
        v += __shfl_xor(v, off, 16);
    return v;
}

__device__ __forceinline__ float group16_reduce_max(float v) {
    #pragma unroll
    for (int off = 8; off > 0; off >>= 1)
        v = fmaxf(v, __shfl_xor(v, off, 16));
    return v;
}

// whole-wave MoE gate (reference OP_SOFTMAX + OP_MOE_GATE,
// nn-cpu-ops.cpp:595-720,1462-1492): softmax over the router logits, then
// iterative top-k with smallest-index tie-break, weights normalized by the
// top-k sum. Every lane of the executing wave returns the full idx/weight
// arrays (static-indexed — runtime-indexed locals land in scratch).
// Callable from consumer kernels so the gate costs ~0.3 us of redundant
// VALU per wave instead of its own ~10 us single-workgroup launch.
__device__ __forceinline__ void moe_gate_wave(
        const float *__restrict__ logits, int n_experts, int topk, int lane,
        int *out_idx, float *out_w) {
    const int per = (n_experts + WAVE - 1) / WAVE;
    // fixed-trip unrolled loops: runtime-indexed arrays go to scratch
    float v[16];  // per-lane expert logits (supports n_experts <= 1024)
    float m = -1e30f;
    #pragma unroll
    for (int i = 0; i < 16; i++) {
        const int eidx = lane * per + i;
        v[i] = (i < per && eidx < n_experts) ? logits[eidx] : -1e30f;
        m = fmaxf(m, v[i]);
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        m = fmaxf(m, __shfl_xor(m, off, WAVE));
    float sum = 0.0f;
    #pragma unroll
    for (int i = 0; i < 16; i++) {
        v[i] = (i < per && (lane * per + i) < n_experts) ? __expf(v[i] - m) : 0.0f;
        sum += v[i];
    }
    sum = wave_reduce_sum(sum);
    const float inv = 1.0f / sum;
    // iterative top-k: packed (prob, smallest-index-wins) max per round
    float wsum = 0.0f;
    float chosen[16];  // topk <= 16
    #pragma unroll
    for (int t = 0; t < 16; t++) {
        if (t >= topk) continue;  // guarded full unroll (break blocks unrolling)
        float best = -1.0f;
        int bi = -1;
        #pragma unroll
        for (int i = 0; i < 16; i++) {
            if (i < per && v[i] > best) { best = v[i]; bi = lane * per + i; }
        }
        // wave argmax: (prob, -index) lexicographic via packed compare
        #pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ob = __shfl_xor(best, off, WAVE);
            const int oi = __shfl_xor(bi, off, WAVE);
            if (ob > best || (ob == best && oi >= 0 && (bi < 0 || oi < bi))) {
                best = ob; bi = oi;
            }
        }
        out_idx[t] = bi;
        chosen[t] = best * inv;
        wsum += best * inv;
        // clear the winner (static-index scan, see scratch note above)
        #pragma unroll
        for (int i = 0; i < 16; i++)
            if (lane * per + i == bi) v[i] = -1.0f;
    }
    // normalize by the top-k sum (reference normTopk)
    const float winv = 1.0f / wsum;
    #pragma unroll
    for (int t = 0; t < 16; t++)
        out_w[t] = t < topk ? chosen[t] * winv : 0.0f;
}

// ---------------------------------------------------------------- Q80 block
// One Q80 block held one value per lane by a 32-lane group: the block scale
// d = absmax/127 and this lane's rounded code (kept as float: the caller
// casts it for its own store and sums it for the blocksum). Role of the
// reference quantizeF32toQ80, nn-quants.cpp:67.
struct Q80Lane {
    float qf;  // rintf(v / d), 0 for an all-zero block
    float d;   // block scale
};

// the one quantiser: a value's code and scale, given its block's absmax
__device__ __forceinline__ Q80Lane q80_quant_lane(float v, float amax) {
    const float d = amax / 127.0f;
    const float inv = d > 0.0f ? 1.0f / d : 0.0f;
    return {rintf(v * inv), d};
}

__device__ __forceinline__ Q80Lane q80_quant_group32(float v) {
    return q80_quant_lane(v, group32_reduce_max(fabsf(v)));
}

// 16-lane sibling: lane j of a 16-lane group holds the interleaved pair
// (2j, 2j+1) of the block (llama rope). Both codes share the block scale.
struct Q80Pair {
    float qf0, qf1;  // codes of elements 2j and 2j+1
    float d;         // block scale
};

__device__ __forceinline__ Q80Pair q80_quant_group16x2(float v0, float v1) {
    const float amax = group16_reduce_max(fmaxf(fabsf(v0), fabsf(v1)));
    const Q80Lane c0 = q80_quant_lane(v0, amax);
    return {c0.qf, q80_quant_lane(v1, amax).qf, c0.d};
}

// ---------------------------------------------------------------- Q80 wire
// TP sync payload per row: n int8 codes, then n/32 f16 block scales stored
// as two bytes each (the row has no 2-byte alignment), no blocksums.
__device__ __forceinline__ void wire_store_scale(uint8_t *row, int n, int jb,
                                                 float d) {
    const __half h = __float2half(d);
    const uint16_t u = *reinterpret_cast<const uint16_t *>(&h);
    row[n + 2 * jb] = (uint8_t)(u & 0xFF);
    row[n + 2 * jb + 1] = (uint8_t)(u >> 8);
}

// acc + dequant(row[c])
__device__ __forceinline__ float wire_load_fma(const uint8_t *row, int n, int c,
                                               float acc) {
    const int8_t qv = (int8_t)row[c];
    const uint16_t u = (uint16_t)row[n + 2 * (c / QB)]
                     | ((uint16_t)row[n + 2 * (c / QB) + 1] << 8);
    const __half h = *reinterpret_cast<const __half *>(&u);
    return fmaf((float)qv, __half2float(h), acc);
}

// ---------------------------------------------------------------- ssq slots
// A residual row's sum of squares is accumulated by whichever kernel last
// wrote the row, so the next rmsnorm needs no reduction. The accumulator of
// batch row b is spread over SSQ_SPREAD slots, one cacheline each: a
// single-address atomicAdd from every workgroup serializes on one cacheline
// (measured: doubled the 4096-row GEMV). Producers add into ssq_slot(),
// consumers read ssq_total().
__device__ __forceinline__ float *ssq_slot(float *ssq, int b, unsigned blk) {
    return ssq + (b * SSQ_SPREAD + (blk & (SSQ_SPREAD - 1))) * SSQ_PAD;
}

// workgroup sum of a per-thread partial into this workgroup's slot of row b:
// wave reduce, per-wave sums staged in LDS, thread 0 adds them in wave order
// and issues the workgroup's one atomic. NW = waves per workgroup of the
// calling kernel's launch, 0 = read it from blockDim (up to 16). Contains a
// barrier: every thread must call it.
template <int NW>
__device__ __forceinline__ void ssq_block_add(float *ssq, int b, float local) {
    local = wave_reduce_sum(local);
    __shared__ float red[NW ? NW : 16];
    const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (lane == 0) red[wid] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        if constexpr (NW != 0) {
            #pragma unroll
            for (int i = 0; i < NW; i++) t += red[i];
        } else {
            for (int i = 0; i < blockDim.x / WAVE; i++) t += red[i];
        }
        atomicAdd(ssq_slot(ssq, b, blockIdx.x), t);
    }
}

__device__ __forceinline__ float ssq_total(const float *ssq, int b) {
    float t = 0.0f;
    #pragma unroll
    for (int k = 0; k < SSQ_SPREAD; k++)
        t += ssq[(b * SSQ_SPREAD + k) * SSQ_PAD];
    return t;
}

// wave-parallel variant: the 16 spread slots live on 16 different
// cachelines (by design — atomics), so the serial loop above costs ~16
// dependent-ish loads at every wave's kernel start; here lanes 0..15 each
// load one slot and a 16-group reduce + broadcast distributes the sum
// (used by the PRO consumers, which run on every wave of 3.5k workgroups)
__device__ __forceinline__ float ssq_total_wave(const float *ssq, int b,
                                                int lane) {
    float t = (lane & 63) < SSQ_SPREAD
                  ? ssq[(b * SSQ_SPREAD + (lane & 15)) * SSQ_PAD] : 0.0f;
    #pragma unroll
    for (int off = 8; off > 0; off >>= 1)
        t += __shfl_xor(t, off, 16);
    return __shfl(t, 0, WAVE);
}

// KV-cache dtype helpers (f16 KV is the default; torch extensions build
// with __HIP_NO_HALF_CONVERSIONS__, so conversions must be explicit). A Q80
// cache (int8 code plane + f16 scale plane per K and V) is opt-in.
__device__ __forceinline__ float kv_f(float v) { return v; }
__device__ __forceinline__ float kv_f(__half v) { return __half2float(v); }
// a Q80 cache code: the block scale is applied by the caller, once per run
__device__ __forceinline__ float kv_f(int8_t v) { return (float)v; }
template <typename T> __device__ __forceinline__ T kv_c(float v);
template <> __device__ __forceinline__ float kv_c<float>(float v) { return v; }
template <> __device__ __forceinline__ __half kv_c<__half>(float v) { return __float2half(v); }

// argmax pack: monotonic unsigned ordering of (float value, smallest index
// wins ties) for a single global atomicMax — on-device greedy sampling.
__device__ __forceinline__ unsigned long long argmax_pack(float v, int idx) {
    unsigned u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned)(0x7FFFFFFF - idx);
}

#define CHECK_CUDA(x) TORCH_CHECK((x).is_cuda(), #x " must be a GPU tensor")
#define CHECK_CONT(x) TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")

static inline hipStream_t cur_stream() {
    return at::hip::getCurrentHIPStream().stream();
}

// one per family source file; module.hip calls them all
void register_quant_norm(py::module &m);
void register_gemv(py::module &m);
void register_gemm(py::module &m);
void register_attn(py::module &m);
void register_moe(py::module &m);
void register_sync(py::module &m);
void register_sampler(py::module &m);
void register_logprob(py::module &m);
void register_host(py::module &m);
