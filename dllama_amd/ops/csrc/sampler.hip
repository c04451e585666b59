// dllama_amd — on-device temperature / top-p sampler (the sampled counterpart
// of k_token_from_argmax), capturable in the decode graph.
//
// Selection rule = Sampler.sample's numpy path (reference
// src/tokenizer.cpp:392-512): p = softmax(logits / T); multinomial when
// topp is outside (0, 1), else nucleus over the candidates with
// p >= (1 - topp) / (V - 1), ordered by descending p (lower index first on
// equal p). coin, temperature and topp are read from device memory
// (params, 3 doubles), so a captured graph follows per-request changes.
//
// Three launches, the kernel boundaries being the only cross-workgroup
// synchronisation:
//   A k_sampler_reduce  one workgroup per SAMPLER_CHUNK logits: local max,
//                       sum-exp and packed argmax -> per-block partials
//   B k_sampler_filter  same grid: every workgroup recombines the partials
//                       (one wave, fixed order: identical M, S everywhere),
//                       recomputes p, appends the candidates as sort keys
//                       (one atomicAdd per workgroup) and writes its sum of
//                       p (vocabulary-order block sums, multinomial mode)
//   C k_sampler_finish  one workgroup: bitonic sort of the candidates in
//                       LDS (padded to the next power of two of their
//                       count), scan, pick; or block-sum scan + in-block scan
//                       (multinomial); or argmax reduce (T == 0). Writes
//                       sample_out {token, status} and re-zeroes the counter.
// A key carries the index, so the arbitrary append order never shows.

#include "dllama_common.h"

#define SAMPLER_MAX_CAND 8192     // 8 B keys: stage C's LDS is exactly 64 KB
#define SAMPLER_THREADS 256
#define SAMPLER_PER_THREAD 4
#define SAMPLER_CHUNK (SAMPLER_THREADS * SAMPLER_PER_THREAD)
#define SAMPLER_FIN_THREADS 1024
#define SAMPLER_FIN_WAVES (SAMPLER_FIN_THREADS / WAVE)
#define SAMPLER_FIN_KEYS (SAMPLER_MAX_CAND / SAMPLER_FIN_THREADS)
#define SAMPLER_NONE 0x7FFFFFFF

typedef unsigned long long u64;

__device__ __forceinline__ float wave_reduce_max(float v) {
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = fmaxf(v, __shfl_xor(v, off, WAVE));
    return v;
}

__device__ __forceinline__ u64 wave_reduce_max_u64(u64 v) {
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = max(v, (u64)__shfl_xor((long long)v, off, WAVE));
    return v;
}

// Global softmax max M and denominator S from the per-block (max, sum-exp)
// partials. Wave 0 alone combines them, lanes striding over the blocks and
// an xor-shuffle tree on top: the order depends on nothing but nblk, so
// stage B's workgroups and stage C all get the same bits. bc = 2 LDS floats.
// Contains barriers: every thread must call it.
__device__ __forceinline__ void sampler_combine(const float *__restrict__ part,
                                                int nblk, float *bc,
                                                float &M, float &S) {
    if (threadIdx.x < WAVE) {
        float m = -INFINITY;
        for (int b = threadIdx.x; b < nblk; b += WAVE)
            m = fmaxf(m, part[2 * b]);
        m = wave_reduce_max(m);
        float s = 0.0f;
        for (int b = threadIdx.x; b < nblk; b += WAVE)
            s = fmaf(part[2 * b + 1], expf(part[2 * b] - m), s);
        s = wave_reduce_sum(s);
        if (threadIdx.x == 0) { bc[0] = m; bc[1] = s; }
    }
    __syncthreads();
    M = bc[0];
    S = bc[1];
    __syncthreads();
}

// ------------------------------------------------------------------ stage A
__global__ __launch_bounds__(SAMPLER_THREADS)
void k_sampler_reduce(const float *__restrict__ logits, int V,
                      const double *__restrict__ params,
                      float *__restrict__ part, u64 *__restrict__ amax) {
    const float T = (float)params[1];
    const bool greedy = T == 0.0f;
    const int base = blockIdx.x * SAMPLER_CHUNK + threadIdx.x;
    float v[SAMPLER_PER_THREAD];
    float m = -INFINITY;
    u64 best = 0ull;
    #pragma unroll
    for (int it = 0; it < SAMPLER_PER_THREAD; it++) {
        const int i = base + it * SAMPLER_THREADS;
        v[it] = -INFINITY;
        if (i < V) {
            const float x = logits[i];
            best = max(best, argmax_pack(x, i));
            v[it] = greedy ? x : x / T;
        }
        m = fmaxf(m, v[it]);
    }
    __shared__ float red[SAMPLER_THREADS / WAVE];
    __shared__ u64 redb[SAMPLER_THREADS / WAVE];
    const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    m = wave_reduce_max(m);
    best = wave_reduce_max_u64(best);
    if (lane == 0) { red[wid] = m; redb[wid] = best; }
    __syncthreads();
    m = red[0];
    best = redb[0];
    #pragma unroll
    for (int w = 1; w < SAMPLER_THREADS / WAVE; w++) {
        m = fmaxf(m, red[w]);
        best = max(best, redb[w]);
    }
    __syncthreads();
    float s = 0.0f;
    #pragma unroll
    for (int it = 0; it < SAMPLER_PER_THREAD; it++)
        s += v[it] == -INFINITY ? 0.0f : expf(v[it] - m);
    s = wave_reduce_sum(s);
    if (lane == 0) red[wid] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        s = red[0];
        #pragma unroll
        for (int w = 1; w < SAMPLER_THREADS / WAVE; w++) s += red[w];
        part[2 * blockIdx.x] = m;
        part[2 * blockIdx.x + 1] = s;
        amax[blockIdx.x] = best;
    }
}

// ------------------------------------------------------------------ stage B
__global__ __launch_bounds__(SAMPLER_THREADS)
void k_sampler_filter(const float *__restrict__ logits, int V,
                      const double *__restrict__ params,
                      const float *__restrict__ part, int nblk,
                      float *__restrict__ bsum, u64 *__restrict__ cand,
                      int *__restrict__ counter) {
    const float T = (float)params[1];
    if (T == 0.0f) return;  // greedy: stage C reduces the argmax partials
    const double topp = params[2];
    const bool nucleus = topp > 0.0 && topp < 1.0;
    const float cutoff = (float)((1.0 - topp) / (double)(V - 1));
    __shared__ float bc[2];
    __shared__ float red[SAMPLER_THREADS / WAVE];
    __shared__ int cnt[SAMPLER_THREADS / WAVE];
    __shared__ int s_base;
    float M, S;
    sampler_combine(part, nblk, bc, M, S);

    const int base = blockIdx.x * SAMPLER_CHUNK + threadIdx.x;
    const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    float p[SAMPLER_PER_THREAD];
    u64 mask[SAMPLER_PER_THREAD];
    float lsum = 0.0f;
    int wcnt = 0;
    #pragma unroll
    for (int it = 0; it < SAMPLER_PER_THREAD; it++) {
        const int i = base + it * SAMPLER_THREADS;
        p[it] = i < V ? expf(logits[i] / T - M) / S : 0.0f;
        lsum += p[it];
        mask[it] = __ballot(nucleus && i < V && p[it] >= cutoff);
        wcnt += __popcll(mask[it]);
    }
    lsum = wave_reduce_sum(lsum);
    if (lane == 0) { red[wid] = lsum; cnt[wid] = wcnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = red[0];
        int total = cnt[0];
        #pragma unroll
        for (int w = 1; w < SAMPLER_THREADS / WAVE; w++) {
            s += red[w];
            total += cnt[w];
        }
        bsum[blockIdx.x] = s;
        // the counter keeps counting past the cap: stage C reads the true
        // candidate count and reports the overflow
        s_base = total ? atomicAdd(counter, total) : 0;
    }
    __syncthreads();
    int pos = s_base;
    #pragma unroll
    for (int w = 0; w < SAMPLER_THREADS / WAVE; w++)
        if (w < wid) pos += cnt[w];
    const u64 below = (1ull << lane) - 1ull;
    #pragma unroll
    for (int it = 0; it < SAMPLER_PER_THREAD; it++) {
        const int i = base + it * SAMPLER_THREADS;
        const int at = pos + __popcll(mask[it] & below);
        if (((mask[it] >> lane) & 1ull) && at < SAMPLER_MAX_CAND)
            cand[at] = ((u64)__float_as_uint(p[it]) << 32)
                     | (unsigned)(0x7FFFFFFF - i);
        pos += __popcll(mask[it]);
    }
}

// ------------------------------------------------------------------ stage C
// Exclusive prefix of v over the 1024 threads in thread order (+ the grand
// total). wtot = SAMPLER_FIN_WAVES LDS floats. Contains barriers.
__device__ __forceinline__ float fin_scan_excl(float v, float *wtot,
                                               float &total) {
    const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    float x = v;
    #pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const float y = __shfl_up(x, off, WAVE);
        if (lane >= off) x += y;
    }
    if (lane == WAVE - 1) wtot[wid] = x;
    const float up = __shfl_up(x, 1, WAVE);
    const float wexcl = lane ? up : 0.0f;
    __syncthreads();
    float pre = 0.0f, tot = 0.0f;
    #pragma unroll
    for (int w = 0; w < SAMPLER_FIN_WAVES; w++) {
        if (w < wid) pre += wtot[w];
        tot += wtot[w];
    }
    __syncthreads();
    total = tot;
    return pre + wexcl;
}

// min over the workgroup of v (SAMPLER_NONE = no vote). slot = 1 LDS int.
__device__ __forceinline__ int fin_min(int v, int *slot) {
    if (threadIdx.x == 0) *slot = SAMPLER_NONE;
    __syncthreads();
    if (v != SAMPLER_NONE) atomicMin(slot, v);
    __syncthreads();
    const int r = *slot;
    __syncthreads();
    return r;
}

// R consecutive levels (compare distances S << (R-1) .. S) of bitonic phase
// k in one pass over the LDS keys: a thread holds the 2^R keys of one
// butterfly group in registers, so a phase of log2(k) levels costs
// ceil(log2(k) / 3) barriers and LDS round trips, not log2(k). The group
// spans 2^R * S <= k keys: one direction for all of it. Ends in a barrier.
template <int R>
__device__ __forceinline__ void bitonic_pass(u64 *keys, int npad, int k, int S) {
    constexpr int E = 1 << R;
    for (int t = threadIdx.x; t < (npad >> R); t += SAMPLER_FIN_THREADS) {
        const int i0 = ((t & ~(S - 1)) << R) | (t & (S - 1));
        const bool desc = (i0 & k) == 0;
        u64 x[E];
        #pragma unroll
        for (int e = 0; e < E; e++) x[e] = keys[i0 + e * S];
        #pragma unroll
        for (int h = E >> 1; h > 0; h >>= 1) {
            #pragma unroll
            for (int e = 0; e < E; e++) {
                if ((e & h) == 0) {
                    const u64 a = x[e], b = x[e | h];
                    const bool sw = (a < b) == desc;
                    x[e] = sw ? b : a;
                    x[e | h] = sw ? a : b;
                }
            }
        }
        #pragma unroll
        for (int e = 0; e < E; e++) keys[i0 + e * S] = x[e];
    }
    __syncthreads();
}

__global__ __launch_bounds__(SAMPLER_FIN_THREADS)
void k_sampler_finish(const float *__restrict__ logits, int V,
                      const double *__restrict__ params,
                      const float *__restrict__ part,
                      const u64 *__restrict__ amax,
                      const float *__restrict__ bsum, int nblk,
                      const u64 *__restrict__ cand, int *__restrict__ counter,
                      long *__restrict__ out) {
    // the sort keys fill the 64 KB; once the sorted keys sit in registers
    // (and in the modes that never sort) its head is the reduction scratch
    __shared__ u64 keys[SAMPLER_MAX_CAND];
    float *wtot = reinterpret_cast<float *>(keys);             // 16 floats
    float *bc = wtot + SAMPLER_FIN_WAVES;                      // 2 floats
    int *slot = reinterpret_cast<int *>(bc + 2);               // 1 int
    float *fslot = reinterpret_cast<float *>(slot + 1);        // 1 float
    u64 *redb = keys + 16;                                     // 16 u64
    const int tid = threadIdx.x;
    const int wid = tid / WAVE, lane = tid % WAVE;
    const float coin = (float)params[0];
    const float T = (float)params[1];
    const double topp = params[2];

    if (T == 0.0f) {  // argmax, lowest index on ties
        u64 best = 0ull;
        for (int b = tid; b < nblk; b += SAMPLER_FIN_THREADS)
            best = max(best, amax[b]);
        best = wave_reduce_max_u64(best);
        if (lane == 0) redb[wid] = best;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < SAMPLER_FIN_WAVES; w++)
                best = max(best, redb[w]);
            out[0] = (long)(0x7FFFFFFF - (int)(best & 0xFFFFFFFFu));
            out[1] = 0;
        }
        return;
    }

    if (!(topp > 0.0 && topp < 1.0)) {
        // multinomial: first index in vocabulary order whose running sum
        // exceeds coin. Scan the per-block sums, then the one block.
        float M, S;
        sampler_combine(part, nblk, bc, M, S);
        float carry = 0.0f, prefix = 0.0f;
        int hit_blk = SAMPLER_NONE;
        for (int b0 = 0; b0 < nblk; b0 += SAMPLER_FIN_THREADS) {
            const int b = b0 + tid;
            const float v = b < nblk ? bsum[b] : 0.0f;
            float total;
            const float excl = carry + fin_scan_excl(v, wtot, total);
            const bool hit = b < nblk && excl + v > coin;
            hit_blk = fin_min(hit ? b : SAMPLER_NONE, slot);
            if (hit_blk != SAMPLER_NONE) {
                if (b == hit_blk) *fslot = excl;
                __syncthreads();
                prefix = *fslot;
                __syncthreads();
                break;
            }
            carry += total;
        }
        int token = V - 1;
        if (hit_blk != SAMPLER_NONE) {
            const int i = hit_blk * SAMPLER_CHUNK + tid;
            const float p = i < V ? expf(logits[i] / T - M) / S : 0.0f;
            float total;
            const float excl = prefix + fin_scan_excl(p, wtot, total);
            const int first = fin_min(i < V && excl + p > coin ? i : SAMPLER_NONE,
                                      slot);
            // the block sum said yes, the finer scan may round to no: the
            // block's last index then
            token = first != SAMPLER_NONE
                        ? first : min(V, (hit_blk + 1) * SAMPLER_CHUNK) - 1;
        }
        if (tid == 0) { out[0] = token; out[1] = 0; }
        return;
    }

    // nucleus
    const int n = *counter;
    __syncthreads();  // every thread has read the count before it is reset
    if (tid == 0) *counter = 0;
    if (n > SAMPLER_MAX_CAND || n <= 0) {
        if (tid == 0) out[1] = 1;  // the caller resamples with the same coin
        return;
    }
    int npad = 1;
    while (npad < n) npad <<= 1;
    for (int i = tid; i < npad; i += SAMPLER_FIN_THREADS)
        keys[i] = i < n ? cand[i] : 0ull;
    __syncthreads();
    // bitonic sort, descending (a padding key 0 sorts last), three levels
    // of a phase per barrier
    for (int k = 2; k <= npad; k <<= 1) {
        int j = k >> 1;
        while (j > 0) {
            if (j >= 4) { bitonic_pass<3>(keys, npad, k, j >> 2); j >>= 3; }
            else if (j == 2) { bitonic_pass<2>(keys, npad, k, 1); j = 0; }
            else { bitonic_pass<1>(keys, npad, k, 1); j = 0; }
        }
    }
    // thread t owns the sorted positions t*8 .. t*8+7
    u64 key[SAMPLER_FIN_KEYS];
    float c[SAMPLER_FIN_KEYS];
    const int p0 = tid * SAMPLER_FIN_KEYS;
    float run = 0.0f;
    #pragma unroll
    for (int j = 0; j < SAMPLER_FIN_KEYS; j++) {
        key[j] = p0 + j < n ? keys[p0 + j] : 0ull;
        run += __uint_as_float((unsigned)(key[j] >> 32));
        c[j] = run;
    }
    __syncthreads();  // keys[] is scratch from here on
    float total;
    const float excl = fin_scan_excl(run, wtot, total);
    int vote = SAMPLER_NONE;
    #pragma unroll
    for (int j = SAMPLER_FIN_KEYS - 1; j >= 0; j--) {
        c[j] += excl;
        if (p0 + j < n && (double)c[j] > topp) vote = p0 + j;
    }
    int last = fin_min(vote, slot);
    if (last == SAMPLER_NONE) last = n - 1;
    #pragma unroll
    for (int j = 0; j < SAMPLER_FIN_KEYS; j++)
        if (p0 + j == last) *fslot = c[j];
    __syncthreads();
    const float r = coin * *fslot;
    __syncthreads();
    vote = SAMPLER_NONE;
    #pragma unroll
    for (int j = SAMPLER_FIN_KEYS - 1; j >= 0; j--)
        if (p0 + j <= last && r < c[j]) vote = p0 + j;
    int pick = fin_min(vote, slot);
    if (pick == SAMPLER_NONE) pick = last;
    #pragma unroll
    for (int j = 0; j < SAMPLER_FIN_KEYS; j++)
        if (p0 + j == pick) {
            out[0] = (long)(0x7FFFFFFF - (int)(key[j] & 0xFFFFFFFFu));
            out[1] = 0;
        }
}

// ------------------------------------------------------------------ host
int64_t sampler_max_candidates() { return SAMPLER_MAX_CAND; }

// workgroups of stages A and B = entries of the per-block scratch
int64_t sampler_blocks(int64_t vocab_size) {
    return ceil_div(vocab_size, SAMPLER_CHUNK);
}

// logits: contiguous f32, the first vocab_size entries count. params: f64
// {coin, temperature, topp} on device. Scratch: part f32 [2*blocks], amax
// i64 [blocks], bsum f32 [blocks], cand i64 [max_candidates], counter i32
// [1] (zero before the first call; stage C leaves it zero). out: i64
// {token, status}; status 1 = more candidates than the cap, no token.
void sample_logits(torch::Tensor logits, int64_t vocab_size, torch::Tensor params,
                   torch::Tensor part, torch::Tensor amax, torch::Tensor bsum,
                   torch::Tensor cand, torch::Tensor counter, torch::Tensor out) {
    CHECK_CUDA(logits); CHECK_CONT(logits);
    CHECK_CUDA(params); CHECK_CUDA(part); CHECK_CUDA(amax); CHECK_CUDA(bsum);
    CHECK_CUDA(cand); CHECK_CUDA(counter); CHECK_CUDA(out);
    CHECK_CONT(params); CHECK_CONT(part); CHECK_CONT(amax); CHECK_CONT(bsum);
    CHECK_CONT(cand); CHECK_CONT(counter); CHECK_CONT(out);
    TORCH_CHECK(logits.scalar_type() == torch::kFloat32, "logits must be f32");
    TORCH_CHECK(vocab_size >= 2 && vocab_size <= logits.numel()
                && vocab_size < (1ll << 31) - SAMPLER_CHUNK,
                "vocab_size out of range for the logits row");
    const int V = (int)vocab_size;
    const int nblk = (int)sampler_blocks(vocab_size);
    TORCH_CHECK(params.scalar_type() == torch::kFloat64 && params.numel() >= 3,
                "params must be f64 {coin, temperature, topp}");
    TORCH_CHECK(part.scalar_type() == torch::kFloat32 && part.numel() >= 2 * nblk
                && bsum.scalar_type() == torch::kFloat32 && bsum.numel() >= nblk
                && amax.scalar_type() == torch::kInt64 && amax.numel() >= nblk,
                "sampler per-block scratch too small for vocab_size");
    TORCH_CHECK(cand.scalar_type() == torch::kInt64
                && cand.numel() >= SAMPLER_MAX_CAND, "cand too small");
    TORCH_CHECK(counter.scalar_type() == torch::kInt32 && counter.numel() >= 1
                && out.scalar_type() == torch::kInt64 && out.numel() >= 2,
                "counter must be i32 [1], out i64 [2]");
    const float *lp = logits.data_ptr<float>();
    const double *pp = params.data_ptr<double>();
    float *partp = part.data_ptr<float>();
    float *bsp = bsum.data_ptr<float>();
    u64 *amp = reinterpret_cast<u64 *>(amax.data_ptr<int64_t>());
    u64 *cp = reinterpret_cast<u64 *>(cand.data_ptr<int64_t>());
    int *cnt = counter.data_ptr<int>();
    hipLaunchKernelGGL(k_sampler_reduce, dim3(nblk), dim3(SAMPLER_THREADS), 0,
                       cur_stream(), lp, V, pp, partp, amp);
    hipLaunchKernelGGL(k_sampler_filter, dim3(nblk), dim3(SAMPLER_THREADS), 0,
                       cur_stream(), lp, V, pp, partp, nblk, bsp, cp, cnt);
    hipLaunchKernelGGL(k_sampler_finish, dim3(1), dim3(SAMPLER_FIN_THREADS), 0,
                       cur_stream(), lp, V, pp, partp, amp, bsp, nblk, cp, cnt,
                       (long *)out.data_ptr<int64_t>());
}

void register_sampler(py::module &m) {
    m.def("sampler_max_candidates", &sampler_max_candidates);
    m.def("sampler_blocks", &sampler_blocks);
    m.def("sample_logits", &sample_logits);
}
