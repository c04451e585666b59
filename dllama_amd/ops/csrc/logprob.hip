// dllama_amd — token log-probabilities from logits that stay on device:
// per row the log-sum-exp, the log-probability of one given token and the K
// most likely tokens with theirs. Capturable: it runs behind the sampler in
// the decode graph and in the row-step graphs.
//
// logprob(i) = logits[i] - logsumexp(logits[:V]): the model's distribution
// at temperature 1, before top-p, whatever the request samples with.
// Order of the top list: descending logit, lower index first on equal
// values (-0.0 and +0.0 are equal: canonicalised before packing).
//
// Two launches for all B rows together, the kernel boundary being the only
// cross-workgroup synchronisation (no atomics, nothing exchanged inside a
// launch), every reduction in an order fixed by the shape alone, so the
// same input gives the same bits:
//   A k_logprob_partial  grid (chunks, B), one workgroup per LOGPROB_CHUNK
//                        logits of one row: the chunk's max, sum-exp and its
//                        top-k packed keys (k rounds of packed max with
//                        knock-out over the keys held in registers)
//   B k_logprob_finish   one workgroup per row: combines the (max, sum-exp)
//                        partials as sampler_combine does (one wave, lanes
//                        striding over the chunks, xor tree), selects the
//                        top-k of the chunks*k keys in LDS by the same
//                        knock-out rounds, reads logits[target], writes
//                        {lse, logprob(target), top-k} and the ids.
// A log-probability is (logit - M) - log(S), never logit - lse: the first
// difference is exact or half an ulp of the row's spread, where lse itself
// can be as large as the logits are.

#include "dllama_common.h"

#define LOGPROB_MAXK 20
#define LOGPROB_THREADS 256
#define LOGPROB_WAVES (LOGPROB_THREADS / WAVE)
#define LOGPROB_PER_THREAD 4
#define LOGPROB_CHUNK (LOGPROB_THREADS * LOGPROB_PER_THREAD)  // = SAMPLER_CHUNK
#define LOGPROB_MAX_KEYS 6144  // stage B's LDS keys: 48 KB of 8 B keys

typedef unsigned long long u64;

__device__ __forceinline__ float lp_wave_max(float v) {
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = fmaxf(v, __shfl_xor(v, off, WAVE));
    return v;
}

__device__ __forceinline__ u64 lp_wave_max_u64(u64 v) {
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = max(v, (u64)__shfl_xor((long long)v, off, WAVE));
    return v;
}

// the key of (value, index): argmax_pack of the value with -0.0 made +0.0,
// so equal values order by index alone. Never 0: 0 marks "no key".
__device__ __forceinline__ u64 lp_key(float x, int i) {
    return argmax_pack(x == 0.0f ? 0.0f : x, i);
}

__device__ __forceinline__ float lp_key_value(u64 key) {
    const unsigned u = (unsigned)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

__device__ __forceinline__ int lp_key_index(u64 key) {
    return 0x7FFFFFFF - (int)(key & 0xFFFFFFFFu);
}

// The workgroup's maximum of `mine` (every thread gets it). red: 2 *
// LOGPROB_WAVES keys, double-buffered by `round`, so that consecutive calls
// need one barrier each: a thread that writes buffer b again has passed the
// barrier of the call between, which every thread reaches only after it has
// read buffer b.
__device__ __forceinline__ u64 lp_block_max(u64 mine, u64 *red, int round) {
    u64 *buf = red + (round & 1) * LOGPROB_WAVES;
    const u64 w = lp_wave_max_u64(mine);
    if (threadIdx.x % WAVE == 0) buf[threadIdx.x / WAVE] = w;
    __syncthreads();
    u64 best = buf[0];
    #pragma unroll
    for (int i = 1; i < LOGPROB_WAVES; i++) best = max(best, buf[i]);
    return best;
}

// ------------------------------------------------------------------ stage A
__global__ __launch_bounds__(LOGPROB_THREADS)
void k_logprob_partial(const float *__restrict__ logits, long row_stride,
                       int V, int k, int nchunk,
                       float *__restrict__ part, u64 *__restrict__ ckeys) {
    const int row = blockIdx.y, chunk = blockIdx.x;
    const float *x = logits + row * row_stride;
    const int base = chunk * LOGPROB_CHUNK + threadIdx.x;
    const int wid = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    __shared__ float red[LOGPROB_WAVES];
    __shared__ u64 redk[2 * LOGPROB_WAVES];
    float v[LOGPROB_PER_THREAD];
    u64 key[LOGPROB_PER_THREAD];
    float m = -INFINITY;
    #pragma unroll
    for (int it = 0; it < LOGPROB_PER_THREAD; it++) {
        const int i = base + it * LOGPROB_THREADS;
        v[it] = -INFINITY;
        key[it] = 0ull;
        if (i < V) {
            v[it] = x[i];
            key[it] = lp_key(v[it], i);
        }
        m = fmaxf(m, v[it]);
    }
    m = lp_wave_max(m);
    if (lane == 0) red[wid] = m;
    __syncthreads();
    m = red[0];
    #pragma unroll
    for (int w = 1; w < LOGPROB_WAVES; w++) m = fmaxf(m, red[w]);
    __syncthreads();
    float s = 0.0f;
    #pragma unroll
    for (int it = 0; it < LOGPROB_PER_THREAD; it++)
        s += v[it] == -INFINITY ? 0.0f : expf(v[it] - m);
    s = wave_reduce_sum(s);
    if (lane == 0) red[wid] = s;
    __syncthreads();
    const long slot = (long)row * nchunk + chunk;
    if (threadIdx.x == 0) {
        s = red[0];
        #pragma unroll
        for (int w = 1; w < LOGPROB_WAVES; w++) s += red[w];
        part[2 * slot] = m;
        part[2 * slot + 1] = s;
    }
    // the chunk's k largest keys, descending; 0 once the chunk has no more
    for (int r = 0; r < k; r++) {
        u64 mine = key[0];
        #pragma unroll
        for (int it = 1; it < LOGPROB_PER_THREAD; it++) mine = max(mine, key[it]);
        const u64 best = lp_block_max(mine, redk, r);
        if (threadIdx.x == 0) ckeys[slot * LOGPROB_MAXK + r] = best;
        #pragma unroll
        for (int it = 0; it < LOGPROB_PER_THREAD; it++)
            if (key[it] == best) key[it] = 0ull;
    }
}

// ------------------------------------------------------------------ stage B
__global__ __launch_bounds__(LOGPROB_THREADS)
void k_logprob_finish(const float *__restrict__ logits, long row_stride,
                      int V, int k, int nchunk,
                      const long *__restrict__ targets, long target_stride,
                      const float *__restrict__ part,
                      const u64 *__restrict__ ckeys,
                      float *__restrict__ out_lp, int *__restrict__ out_id) {
    const int row = blockIdx.x, tid = threadIdx.x;
    const float *x = logits + row * row_stride;
    const float *rpart = part + 2 * (long)row * nchunk;
    float *lp = out_lp + row * (2 + LOGPROB_MAXK);
    int *id = out_id + row * LOGPROB_MAXK;
    __shared__ float bc[2];
    __shared__ u64 redk[2 * LOGPROB_WAVES];
    __shared__ u64 keys[LOGPROB_MAX_KEYS];

    // M, S as sampler_combine: wave 0, lanes striding over the chunks, xor
    // tree; the order depends on nchunk alone
    if (tid < WAVE) {
        float m = -INFINITY;
        for (int c = tid; c < nchunk; c += WAVE) m = fmaxf(m, rpart[2 * c]);
        m = lp_wave_max(m);
        float s = 0.0f;
        for (int c = tid; c < nchunk; c += WAVE)
            s = fmaf(rpart[2 * c + 1], expf(rpart[2 * c] - m), s);
        s = wave_reduce_sum(s);
        if (tid == 0) { bc[0] = m; bc[1] = s; }
    }
    // thread t owns the keys t, t + 256, ...: nobody else reads or clears
    // them, so the knock-out needs no barrier of its own
    const int n = nchunk * k;  // <= LOGPROB_MAX_KEYS (host check)
    u64 mine = 0ull;
    for (int j = tid; j < n; j += LOGPROB_THREADS) {
        const u64 key = ckeys[((long)row * nchunk + j / k) * LOGPROB_MAXK + j % k];
        keys[j] = key;
        mine = max(mine, key);
    }
    __syncthreads();
    const float M = bc[0], logS = logf(bc[1]);
    if (tid == 0) {
        lp[0] = M + logS;
        const long t = targets[row * target_stride];
        lp[1] = t >= 0 && t < V ? (x[t] - M) - logS : -INFINITY;
    }
    for (int r = 0; r < k; r++) {
        const u64 best = lp_block_max(mine, redk, r);
        if (tid == 0) {
            lp[2 + r] = best ? (lp_key_value(best) - M) - logS : -INFINITY;
            id[r] = best ? lp_key_index(best) : -1;
        }
        if (mine == best && best) {  // the owner: clear it, find its next
            mine = 0ull;
            for (int j = tid; j < n; j += LOGPROB_THREADS) {
                if (keys[j] == best) keys[j] = 0ull;
                mine = max(mine, keys[j]);
            }
        }
    }
    for (int r = k + tid; r < LOGPROB_MAXK; r += LOGPROB_THREADS) {
        lp[2 + r] = -INFINITY;
        id[r] = -1;
    }
}

// ------------------------------------------------------------------ host
int64_t logprob_max_k() { return LOGPROB_MAXK; }

// workgroups per row of stage A = per-row entries of the scratch
int64_t logprob_chunks(int64_t vocab_size) {
    return ceil_div(vocab_size, LOGPROB_CHUNK);
}

// logits: f32 [B, >= vocab_size] or [>= vocab_size] (B = 1), unit element
// stride, any row stride: nothing is copied. targets: i64 [>= B], any
// stride; one outside [0, vocab_size) gives -inf for that row's target
// log-probability and nothing else. k: 0..20. Scratch: part f32
// [2 * B * chunks], keys i64 [20 * B * chunks]. out_lp: f32 [B, 22] = {lse,
// logprob(target), top-k logprobs descending}; out_id: i32 [B, 20]; entries
// past min(k, vocab_size) are -inf / -1.
void logprob_rows(torch::Tensor logits, int64_t vocab_size, torch::Tensor targets,
                  int64_t k, torch::Tensor part, torch::Tensor keys,
                  torch::Tensor out_lp, torch::Tensor out_id) {
    CHECK_CUDA(logits); CHECK_CUDA(targets); CHECK_CUDA(part); CHECK_CUDA(keys);
    CHECK_CUDA(out_lp); CHECK_CUDA(out_id);
    CHECK_CONT(part); CHECK_CONT(keys); CHECK_CONT(out_lp); CHECK_CONT(out_id);
    TORCH_CHECK(logits.scalar_type() == torch::kFloat32
                && (logits.dim() == 1 || logits.dim() == 2)
                && logits.stride(-1) == 1,
                "logits must be f32 [B, V] or [V] with unit element stride");
    const int64_t B = logits.dim() == 2 ? logits.size(0) : 1;
    const int64_t row_stride = logits.dim() == 2 ? logits.stride(0) : 0;
    TORCH_CHECK(B >= 1 && B <= 65535, "1..65535 rows (got ", B, ")");
    TORCH_CHECK(row_stride >= 0, "logits row stride must not be negative");
    TORCH_CHECK(vocab_size >= 2 && vocab_size <= logits.size(-1)
                && vocab_size < (1ll << 31) - LOGPROB_CHUNK,
                "vocab_size out of range for the logits row");
    TORCH_CHECK(k >= 0 && k <= LOGPROB_MAXK, "k must be 0..", LOGPROB_MAXK,
                " (got ", k, ")");
    const int64_t nchunk = logprob_chunks(vocab_size);
    TORCH_CHECK(nchunk * k <= LOGPROB_MAX_KEYS,
                "logprob_rows holds at most ", LOGPROB_MAX_KEYS,
                " chunk keys per row: vocab_size ", vocab_size, " at k = ", k,
                " has ", nchunk * k);
    TORCH_CHECK(targets.scalar_type() == torch::kInt64 && targets.dim() == 1
                && targets.size(0) >= B && targets.stride(0) >= 0,
                "targets must be i64 [>= B]");
    TORCH_CHECK(part.scalar_type() == torch::kFloat32
                && part.numel() >= 2 * B * nchunk
                && keys.scalar_type() == torch::kInt64
                && keys.numel() >= LOGPROB_MAXK * B * nchunk,
                "logprob scratch too small for B rows of vocab_size");
    TORCH_CHECK(out_lp.scalar_type() == torch::kFloat32
                && out_lp.numel() >= B * (2 + LOGPROB_MAXK)
                && out_id.scalar_type() == torch::kInt32
                && out_id.numel() >= B * LOGPROB_MAXK,
                "out_lp must be f32 [B, 22], out_id i32 [B, 20]");
    const float *lp = logits.data_ptr<float>();
    float *partp = part.data_ptr<float>();
    u64 *kp = reinterpret_cast<u64 *>(keys.data_ptr<int64_t>());
    hipLaunchKernelGGL(k_logprob_partial, dim3((unsigned)nchunk, (unsigned)B),
                       dim3(LOGPROB_THREADS), 0, cur_stream(), lp,
                       (long)row_stride, (int)vocab_size, (int)k, (int)nchunk,
                       partp, kp);
    hipLaunchKernelGGL(k_logprob_finish, dim3((unsigned)B),
                       dim3(LOGPROB_THREADS), 0, cur_stream(), lp,
                       (long)row_stride, (int)vocab_size, (int)k, (int)nchunk,
                       (const long *)targets.data_ptr<int64_t>(),
                       (long)targets.stride(0), partp, kp,
                       out_lp.data_ptr<float>(), out_id.data_ptr<int>());
}

void register_logprob(py::module &m) {
    m.def("logprob_max_k", &logprob_max_k);
    m.def("logprob_chunks", &logprob_chunks);
    m.def("logprob_rows", &logprob_rows);
}
