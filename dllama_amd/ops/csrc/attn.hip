// dllama_amd — split-K flash-decode attention, rope and KV-cache writes.

#include "dllama_common.h"

// ------------------------------------------------- row addressing policies
// Which sequence position a batch row is, and where its sequence starts in
// the KV cache. The positional kernels below are templated on one of these;
// all read wave-uniform values (b is a blockIdx), so they stay scalar.
//
// SeqRows: row b is position pos[0]+b of the one cache (a prompt chunk or a
// decode step of a single sequence).
//
// cache_row(b, t) is the cache row of position t of row b's sequence. The
// first two policies keep a sequence in consecutive rows, so attention takes
// cache_base(b) once and adds t itself; PagedRows looks t up per page.
struct SeqRows {
    static constexpr bool kPaged = false;
    const int *pos;
    __device__ int position(int b) const { return pos[0] + b; }
    __device__ int64_t cache_base(int) const { return 0; }
    __device__ int64_t cache_row(int, int t) const { return t; }
};
// TableRows: int32 [B, 2] = {cache_row_base, pos} per row, cache_row_base =
// slot * seq_len: row b is position pos of the sequence whose cache rows
// start at cache_row_base. Expresses N sequences decoding together, a prompt
// chunk into any slot, and any mix of the two.
struct TableRows {
    static constexpr bool kPaged = false;
    const int *rows;
    __device__ int position(int b) const { return rows[2 * b + 1]; }
    __device__ int64_t cache_base(int b) const { return rows[2 * b]; }
    __device__ int64_t cache_row(int b, int t) const {
        return (int64_t)rows[2 * b] + t;
    }
};
// PagedRows: the same [B, 2] table, word 0 now the row's offset into a page
// table (slot * pages_per_seq). The cache is a pool of pages of P = 1<<shift
// rows; position t of row b lives in row pages[offset + t/P] * P + t%P.
struct PagedRows {
    static constexpr bool kPaged = true;
    const int *rows;
    const int *pages;
    int shift;
    __device__ int position(int b) const { return rows[2 * b + 1]; }
    __device__ int64_t cache_base(int) const { return 0; }
    // the page ids of row b's sequence, by page index
    __device__ const int *seq_pages(int b) const { return pages + rows[2 * b]; }
    __device__ int64_t cache_row(int b, int t) const {
        return ((int64_t)seq_pages(b)[t >> shift] << shift)
             + (t & ((1 << shift) - 1));
    }
};

// a lane's run of N consecutive cache elements, loaded as one vector
template <typename T, int N>
struct alignas(sizeof(T) * N) KVPack { T e[N]; };

// ------------------------------------------------- Q80 KV cache
// KVT = int8_t: the cache is a code plane int8 [rows, kv_dim0] and a scale
// plane f16 [rows, kv_dim0/32], both indexed by the same cache row, so every
// addressing policy serves it unchanged. A block is 32 consecutive elements
// of a row (never across a head: head_dim is 64 or 128), value = code *
// f32(scale). The scale planes ride with the addressing policy (Q80Rows), so
// the Q80 forms of the attention kernels are instantiations of the same
// templates and the f16/f32 ones compile to what they were. A lane reads its
// run of codes as one 8-, 4-, 2- or 1-byte load, always inside one block: a
// K run costs one scale load and one multiply on its partial dot, a V run
// folds its scale into the softmax weight.
template <typename KVT>
inline constexpr bool kKVQ80 = std::is_same_v<KVT, int8_t>;

template <typename ROWS>
struct Q80Rows : ROWS {
    const __half *ks;  // K scales, f16 [rows, kv_dim0/32]
    const __half *vs;  // V scales
};

// ------------------------------------------------- split-K flash decode
// Stage 1: grid (H0, B, S); split sp covers t = (sp*4+wave) + 4*S*i — the
// t-range is spread over S*4 waves so long contexts fill the chip.
// Per-split (m, l, o) goes to scratch; stage 2 combines the S partials.
template <int VEC, typename KVT, typename ROWS = SeqRows>
__global__ void k_attn_split(const float *__restrict__ q, int q_ld,
                             const KVT *__restrict__ kc_all,
                             const KVT *__restrict__ vc_all,
                             const ROWS rows,
                             int n_heads0, int kv_mul, int kv_dim0, float scale,
                             float *__restrict__ ml_scratch,
                             float *__restrict__ o_scratch) {
    constexpr bool Q8 = kKVQ80<KVT>;
    [[maybe_unused]] const int nblk = kv_dim0 / QB;  // scales per cache row
    [[maybe_unused]] const __half *ks = nullptr, *vs = nullptr;
    if constexpr (Q8) {
        ks = rows.ks + rows.cache_base(blockIdx.y) * nblk;
        vs = rows.vs + rows.cache_base(blockIdx.y) * nblk;
    }
    const int h0 = blockIdx.x;
    const int b = blockIdx.y;
    const int sp = blockIdx.z;
    const int S = gridDim.z;
    const int hd = VEC * WAVE;
    // the row attends over cache rows base .. base+pos of its own sequence
    const int plen = rows.position(b) + 1;
    const KVT *kc = kc_all + rows.cache_base(b) * kv_dim0;
    const KVT *vc = vc_all + rows.cache_base(b) * kv_dim0;
    // paged: the wave index made provably uniform, so the page-id loads
    // below are scalar loads beside the vector K/V stream
    const int wave = ROWS::kPaged
        ? __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE)
        : threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int kv_off = (h0 / kv_mul) * hd;

    // Each wave's 4 groups of 16 lanes score 4 timesteps per iteration:
    // the serial online-softmax chain advances once per 4 t (a 1-t-per-wave
    // loop measured 22 us at pos=1024 — latency-chained, not memory-bound).
    const int VEC16 = VEC * 4;  // q/k elems per lane within a 16-lane group
    const int lane16 = lane & 15;
    const int group = lane >> 4;

    float qreg[VEC16];
    #pragma unroll
    for (int v = 0; v < VEC16; v++)
        qreg[v] = q[(int64_t)b * q_ld + h0 * hd + lane16 * VEC16 + v] * scale;

    float m = -1e30f, l = 0.0f, o[VEC];
    #pragma unroll
    for (int v = 0; v < VEC; v++) o[v] = 0.0f;

    // 4 t-chunks (16 timesteps) per online-softmax round: the K dots of all
    // 4 chunks are independent, so their HBM loads issue together instead of
    // serializing behind the softmax chain (the 1-chunk-per-round loop was
    // latency-bound: ~13 us at pos 1024 for ~1.3 us of KV traffic)
    const int stride = 16 * S;
    // Paged: chunk u of a round covers t = tb0 + u*stride + 0..3, which
    // starts at a multiple of 4 and so lies in one page for every P >= 4: one
    // page id per chunk, four per round. They are loaded a round ahead, all
    // four together (this round's arrive while the previous round's K/V
    // stream), so the lookup adds no serial hop in front of the K loads. A
    // chunk at or past plen reads no id: its entry may be past the table.
    [[maybe_unused]] int pg[4];
    [[maybe_unused]] const int *seq_pages = nullptr;
    [[maybe_unused]] int pshift = 0;
    if constexpr (ROWS::kPaged) {
        seq_pages = rows.seq_pages(b);
        pshift = rows.shift;
        #pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = (sp * 4 + wave) * 4 + u * stride;
            pg[u] = t < plen ? seq_pages[t >> pshift] : 0;
        }
    }
    for (int tb0 = (sp * 4 + wave) * 4; tb0 < plen; tb0 += 4 * stride) {
        // paged: first cache row of each chunk
        [[maybe_unused]] int64_t rb[4];
        if constexpr (ROWS::kPaged) {
            #pragma unroll
            for (int u = 0; u < 4; u++) {
                const int t = tb0 + u * stride;
                rb[u] = ((int64_t)pg[u] << pshift) + (t & ((1 << pshift) - 1));
            }
            #pragma unroll
            for (int u = 0; u < 4; u++) {
                const int t = tb0 + 4 * stride + u * stride;
                pg[u] = t < plen ? seq_pages[t >> pshift] : 0;
            }
        }
        float su[4];
        #pragma unroll
        for (int u = 0; u < 4; u++) {
            const int tg = tb0 + u * stride + group;
            float partial = 0.0f;
            if (tg < plen) {
                const int64_t kr = ROWS::kPaged ? rb[u] + group : (int64_t)tg;
                const KVT *krow = kc + kr * kv_dim0 + kv_off + lane16 * VEC16;
                if constexpr (Q8) {
                    const auto kk =
                        *reinterpret_cast<const KVPack<KVT, VEC16> *>(krow);
                    const float d = __half2float(
                        ks[kr * nblk + (kv_off + lane16 * VEC16) / QB]);
                    #pragma unroll
                    for (int v = 0; v < VEC16; v++)
                        partial = fmaf(qreg[v], kv_f(kk.e[v]), partial);
                    partial *= d;
                } else {
                    #pragma unroll
                    for (int v = 0; v < VEC16; v++)
                        partial = fmaf(qreg[v], kv_f(krow[v]), partial);
                }
            }
            su[u] = group16_reduce_sum(partial);
        }
        float s16[16];
        float mn = m;
        #pragma unroll
        for (int u = 0; u < 4; u++) {
            #pragma unroll
            for (int gg = 0; gg < 4; gg++) {
                float v = __shfl(su[u], gg * 16, WAVE);
                if (tb0 + u * stride + gg >= plen) v = -1e30f;
                s16[4 * u + gg] = v;
                mn = fmaxf(mn, v);
            }
        }
        const float f = __expf(m - mn);
        float w16[16];
        float lsum = 0.0f;
        #pragma unroll
        for (int i = 0; i < 16; i++) {
            w16[i] = __expf(s16[i] - mn);
            lsum += w16[i];
        }
        l = l * f + lsum;
        #pragma unroll
        for (int v = 0; v < VEC; v++) o[v] *= f;
        #pragma unroll
        for (int u = 0; u < 4; u++) {
            #pragma unroll
            for (int gg = 0; gg < 4; gg++) {
                const int t = tb0 + u * stride + gg;
                if (t >= plen) continue;
                const int64_t vr = ROWS::kPaged ? rb[u] + gg : (int64_t)t;
                const KVT *vrow = vc + vr * kv_dim0 + kv_off + lane * VEC;
                if constexpr (Q8) {
                    const auto vv =
                        *reinterpret_cast<const KVPack<KVT, VEC> *>(vrow);
                    const float wd = w16[4 * u + gg] * __half2float(
                        vs[vr * nblk + (kv_off + lane * VEC) / QB]);
                    #pragma unroll
                    for (int v = 0; v < VEC; v++)
                        o[v] = fmaf(wd, kv_f(vv.e[v]), o[v]);
                } else {
                    #pragma unroll
                    for (int v = 0; v < VEC; v++)
                        o[v] = fmaf(w16[4 * u + gg], kv_f(vrow[v]), o[v]);
                }
            }
        }
        m = mn;
    }

    __shared__ float sm[4], sl[4];
    __shared__ float so[4][VEC * WAVE];
    if (lane == 0) { sm[wave] = m; sl[wave] = l; }
    __syncthreads();
    const float M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    const float fw = __expf(m - M);
    #pragma unroll
    for (int v = 0; v < VEC; v++) so[wave][lane * VEC + v] = o[v] * fw;
    __syncthreads();
    const int64_t slot = ((int64_t)b * n_heads0 + h0) * S + sp;
    if (wave == 0) {
        const float L = sl[0] * __expf(sm[0] - M) + sl[1] * __expf(sm[1] - M)
                      + sl[2] * __expf(sm[2] - M) + sl[3] * __expf(sm[3] - M);
        if (lane == 0) {
            ml_scratch[slot * 2] = M;
            ml_scratch[slot * 2 + 1] = L;
        }
        #pragma unroll
        for (int v = 0; v < VEC; v++) {
            const int i = lane * VEC + v;
            o_scratch[slot * hd + i] = so[0][i] + so[1][i] + so[2][i] + so[3][i];
        }
    }
}

// ------------------------------------------------- wide single-launch decode
// S == 1 with Q80 output, for short contexts: grid (H0, B), one workgroup of
// 16 waves per head, no scratch round trip and no combine launch. A round
// covers 256 consecutive timesteps, t = round*256 + wave*16 + u*4 + group, so
// a decode step below position 256 is ONE round: q, the four K chunks and
// the 16 V rows of a lane are all loaded before the first reduction (the V
// addresses do not depend on the softmax), and the kernel costs about one
// memory latency plus the LDS merge. The 4-wave kernel it replaces covered
// 64 timesteps per round with the V loads behind each round's softmax: about
// nine dependent latencies at position 250, which is what made it slower
// than the split + combine pair. Correct at any plen (further rounds run the
// online softmax per wave); only its speed is tied to short contexts.

// A load of a 2-, 4- or 8-byte pack that the compiler keeps where it is
// written. Plain loads of read-only memory are sunk towards their first use,
// which puts the V loads behind the waits of the K dots; a relaxed atomic
// load of wavefront scope is the same instruction with no cache-policy bits
// and no wait of its own, but it keeps its place among the side effects.
template <int BYTES> struct UIntOfSize;
template <> struct UIntOfSize<2> { using type = unsigned short; };
template <> struct UIntOfSize<4> { using type = unsigned int; };
template <> struct UIntOfSize<8> { using type = unsigned long long; };
template <typename P>
__device__ __forceinline__ typename UIntOfSize<sizeof(P)>::type
load_in_order_raw(const P *p) {
    using U = typename UIntOfSize<sizeof(P)>::type;
    return __hip_atomic_load(reinterpret_cast<const U *>(p), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WAVEFRONT);
}
template <typename P>
__device__ __forceinline__ P load_in_order(const P *p) {
    const auto u = load_in_order_raw(p);
    P r;
    __builtin_memcpy(&r, &u, sizeof(P));
    return r;
}

// The wide kernel's loads of a Q80 cache. A lane's V run is 2 or 1 codes and
// a block scale is 2 bytes, but an in-order load narrower than a dword comes
// with an AND on the loaded value (the zero extension is not folded into an
// atomic load), and any unpack or conversion of a single loaded value is
// placed right behind its load, in front of the sched_barrier, with a wait
// on that load (read in the ISA: a wait per K run before the V loads issue,
// a wait per V row before the first K dot). So:
//  - every such load is the aligned dword that holds the lane's bytes (the
//    2 or 4 lanes that share a dword, the 16 or 32 that share a scale, read
//    one address: no more traffic), kept as the integer it was loaded as;
//  - hold_here() behind the barrier is an empty volatile asm on that
//    register: a side effect, ordered behind the barrier, so the shifts and
//    conversions that pick the lane's bytes stay behind it too.
// Planes, rows and heads all start on dword boundaries: kv_dim0 and the head
// offsets are multiples of 64 codes = 4 scales.
template <typename P>
__device__ __forceinline__ unsigned int load_dword_of(const P *p) {
    // an offset from p, not a masked integer: the address stays global
    const char *c = reinterpret_cast<const char *>(p);
    return load_in_order_raw(reinterpret_cast<const unsigned int *>(
        c - (reinterpret_cast<uintptr_t>(c) & 3)));
}
// a V run as the kernel holds it from load to use: the pack, or for Q80
// codes the dword that holds the run
template <typename T, int N>
__device__ __forceinline__ auto load_v_run(const KVPack<T, N> *p) {
    if constexpr (kKVQ80<T>) return load_dword_of(p);
    else return load_in_order(p);
}
__device__ __forceinline__ unsigned int load_scale_dword(const __half *row,
                                                         int blk) {
    return load_in_order_raw(
        reinterpret_cast<const unsigned int *>(row + (blk & ~1)));
}
__device__ __forceinline__ void hold_here(unsigned int &x) {
    asm volatile("" : "+v"(x));
}
__device__ __forceinline__ void hold_here(unsigned long long &x) {
    asm volatile("" : "+v"(x));
}
template <typename T, int N>
__device__ __forceinline__ void hold_here(KVPack<T, N> &p) {
    typename UIntOfSize<sizeof(p)>::type u;
    __builtin_memcpy(&u, &p, sizeof(p));
    hold_here(u);
    __builtin_memcpy(&p, &u, sizeof(p));
}
// the code `shift` bits up in a dword of codes; the f16 scale likewise
__device__ __forceinline__ float code_at(unsigned int codes, int shift) {
    return (float)(int8_t)(codes >> shift);
}
__device__ __forceinline__ float scale_at(unsigned int scales, int shift) {
    return __half2float(__ushort_as_half((unsigned short)(scales >> shift)));
}


// the 16 (chunk u, row g) pairs of a wave's round: the V rows live in 16
// named registers, not an indexed array the allocator could send to scratch
#define ATTN_WIDE_ROWS(X) \
    X(0, 0) X(0, 1) X(0, 2) X(0, 3) X(1, 0) X(1, 1) X(1, 2) X(1, 3) \
    X(2, 0) X(2, 1) X(2, 2) X(2, 3) X(3, 0) X(3, 1) X(3, 2) X(3, 3)

// Q80 (KVT = int8_t, ROWS = Q80Rows<..>): the round's scale loads (4 for K,
// 16 for V per lane) follow the rules of the K/V loads: issued before the
// sched_barrier, never guarded, and a timestep at or past plen re-reads row
// plen-1, scale included.
template <int VEC, typename KVT, typename ROWS>
__global__ void __launch_bounds__(1024)
k_attn_wide(const float *__restrict__ q, int q_ld,
            const KVT *__restrict__ kc_all,
            const KVT *__restrict__ vc_all,
            const ROWS rows,
            int n_heads0, int kv_mul, int kv_dim0, float scale,
            int8_t *__restrict__ zq,
            float *__restrict__ zs,
            float *__restrict__ zbs) {
    constexpr bool Q8 = kKVQ80<KVT>;
    constexpr int NW = 16;         // waves per workgroup
    constexpr int hd = VEC * WAVE;
    constexpr int VEC16 = VEC * 4;  // q/k elems per lane within a 16-lane group
    using KPack = KVPack<KVT, VEC16>;
    using VPack = KVPack<KVT, VEC>;
    const int h0 = blockIdx.x;
    const int b = blockIdx.y;
    // every row of a row table has its own length
    const int plen = rows.position(b) + 1;
    const KVT *kc = kc_all + rows.cache_base(b) * kv_dim0;
    const KVT *vc = vc_all + rows.cache_base(b) * kv_dim0;
    [[maybe_unused]] const int nblk = kv_dim0 / QB;  // scales per cache row
    [[maybe_unused]] const __half *ks = nullptr, *vs = nullptr;
    if constexpr (Q8) {
        ks = rows.ks + rows.cache_base(b) * nblk;
        vs = rows.vs + rows.cache_base(b) * nblk;
    }
    // provably wave-uniform: the round loop branches on it and every row
    // address below is a wave-uniform base plus a lane offset
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int lane = threadIdx.x % WAVE;
    const int kv_off = (h0 / kv_mul) * hd;
    const int lane16 = lane & 15;
    const int group = lane >> 4;

    // q first; it is scaled on the score so that nothing uses it (and waits
    // for it) before the K and V loads have issued
    float qreg[VEC16];
    #pragma unroll
    for (int v = 0; v < VEC16; v++)
        qreg[v] = q[(int64_t)b * q_ld + h0 * hd + lane16 * VEC16 + v];

    float m = -1e30f, l = 0.0f, o[VEC];
    #pragma unroll
    for (int v = 0; v < VEC; v++) o[v] = 0.0f;

    // A 4-timestep chunk starts at a multiple of 4, so it lies in one page
    // for every page size >= 4: one page id per chunk. hipcc puts a branch
    // and a full wait around every guarded load (20 serial latencies), so no
    // load is guarded: in the one wave per round that straddles plen, a
    // timestep >= plen re-reads row plen-1 of the sequence (always a valid
    // row, and a page id inside the table), is scored -1e30 below and weighs
    // exactly 0.
    const int tlast = plen - 1;
    // paged: the round's four page ids, loaded a round ahead as in
    // k_attn_split; the first round's here, ahead of the loop, where the four
    // issue together (inside it each lookup was a load and a full wait)
    [[maybe_unused]] int pg[4];
    if constexpr (ROWS::kPaged) {
        #pragma unroll
        for (int u = 0; u < 4; u++)
            pg[u] = rows.seq_pages(b)[min(wave * 16 + u * 4, tlast & ~3)
                                      >> rows.shift];
    }

    // a wave whose first timestep is at or past plen never enters: it keeps
    // m = -1e30, l = 0, o = 0 and weighs nothing in the merge
    for (int tb = wave * 16; tb < plen; tb += 16 * NW) {
        int trow[4];      // the chunk's first t, clamped to the last chunk
        int64_t roff[4];  // wave-uniform: where that row's head starts
        [[maybe_unused]] int64_t soff[4];  // Q80: the same in the scale planes
        #pragma unroll
        for (int u = 0; u < 4; u++) {
            trow[u] = min(tb + u * 4, tlast & ~3);
            int64_t r = trow[u];  // kc / vc start at the row's sequence
            if constexpr (ROWS::kPaged)
                r = ((int64_t)pg[u] << rows.shift)
                  + (trow[u] & ((1 << rows.shift) - 1));
            roff[u] = r * kv_dim0 + kv_off;
            if constexpr (Q8) soff[u] = r * nblk + kv_off / QB;
        }
        // all loads of the round, K then V, before anything waits on one
        KPack kk[4];
        // Q80: the dword with the block scale of each K run
        [[maybe_unused]] unsigned int kd[4];
        #pragma unroll
        for (int u = 0; u < 4; u++) {
            const int g = min(trow[u] + group, tlast) - trow[u];
            kk[u] = *reinterpret_cast<const KPack *>(
                kc + roff[u] + (g * kv_dim0 + lane16 * VEC16));
            if constexpr (Q8)
                kd[u] = load_scale_dword(ks + soff[u] + g * nblk,
                                         lane16 * VEC16 / QB);
        }
        #define X(u, g) \
            auto v##u##g = load_v_run(reinterpret_cast<const VPack *>( \
                vc + roff[u] + (min(trow[u] + g, tlast) - trow[u]) * kv_dim0 \
                + lane * VEC)); \
            [[maybe_unused]] unsigned int d##u##g = 0; \
            if constexpr (Q8) \
                d##u##g = load_scale_dword( \
                    vs + soff[u] + (min(trow[u] + g, tlast) - trow[u]) * nblk, \
                    lane * VEC / QB);
        ATTN_WIDE_ROWS(X)
        #undef X
        // nothing moves across this: the V loads stay above the first K wait
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (Q8) {
            #pragma unroll
            for (int u = 0; u < 4; u++) {
                hold_here(kk[u]);
                hold_here(kd[u]);
            }
        }

        float s16[16];
        float mn = m;
        #pragma unroll
        for (int u = 0; u < 4; u++) {
            float partial = 0.0f;
            #pragma unroll
            for (int v = 0; v < VEC16; v++)
                partial = fmaf(qreg[v], kv_f(kk[u].e[v]), partial);
            if constexpr (Q8)
                partial *= scale_at(kd[u], 16 * ((lane16 * VEC16 / QB) & 1));
            const float su = group16_reduce_sum(partial) * scale;
            #pragma unroll
            for (int gg = 0; gg < 4; gg++) {
                float v = __shfl(su, gg * 16, WAVE);
                if (tb + u * 4 + gg >= plen) v = -1e30f;
                s16[4 * u + gg] = v;
                mn = fmaxf(mn, v);
            }
        }
        // tb < plen: the round has a valid timestep, so mn is a real score
        // and a masked one weighs exp(-1e30 - mn) = 0
        const float f = __expf(m - mn);
        float w16[16];
        float lsum = 0.0f;
        #pragma unroll
        for (int i = 0; i < 16; i++) {
            w16[i] = __expf(s16[i] - mn);
            lsum += w16[i];
        }
        l = l * f + lsum;
        #pragma unroll
        for (int v = 0; v < VEC; v++) o[v] *= f;
        if constexpr (Q8) {
            // the V holds come here, behind the K holds and the scores: a
            // hold is a use, and up there it would wait for all 40 loads
            // in front of the first K dot
            #define X(u, g) hold_here(v##u##g); hold_here(d##u##g);
            ATTN_WIDE_ROWS(X)
            #undef X
        }
        #define X(u, g) \
            if constexpr (Q8) { \
                /* where the lane's scale and codes sit in their dwords */ \
                const float w = w16[4 * u + g] \
                    * scale_at(d##u##g, 16 * ((lane * VEC / QB) & 1)); \
                _Pragma("unroll") \
                for (int v = 0; v < VEC; v++) \
                    o[v] = fmaf(w, code_at(v##u##g, \
                                           8 * (((lane * VEC) & 3) + v)), o[v]); \
            } else { \
                _Pragma("unroll") \
                for (int v = 0; v < VEC; v++) \
                    o[v] = fmaf(w16[4 * u + g], kv_f(v##u##g.e[v]), o[v]); \
            }
        ATTN_WIDE_ROWS(X)
        #undef X
        m = mn;
        if constexpr (ROWS::kPaged) {
            #pragma unroll
            for (int u = 0; u < 4; u++)
                pg[u] = rows.seq_pages(b)[min(tb + 16 * NW + u * 4, tlast & ~3)
                                          >> rows.shift];
        }
    }

    // merge the 16 waves: one barrier, then hd threads each sum the 16
    // partials of one output element
    __shared__ float sm[NW], sl[NW];
    __shared__ float so[NW][hd];
    if (lane == 0) { sm[wave] = m; sl[wave] = l; }
    #pragma unroll
    for (int v = 0; v < VEC; v++) so[wave][lane * VEC + v] = o[v];
    __syncthreads();
    if (threadIdx.x >= hd) return;
    const int i = threadIdx.x;
    float M = -1e30f;
    #pragma unroll
    for (int w = 0; w < NW; w++) M = fmaxf(M, sm[w]);
    // wave 0 always has timestep 0, so M is a real score; an empty wave has
    // l = 0 and o = 0 and a weight of exp(-1e30 - M) = 0
    float L = 0.0f, acc = 0.0f;
    #pragma unroll
    for (int w = 0; w < NW; w++) {
        const float fw = __expf(sm[w] - M);
        L = fmaf(sl[w], fw, L);
        acc = fmaf(so[w][i], fw, acc);
    }
    // the Q80 triple of the head: thread i holds element i, so a block is a
    // 32-lane group (hd threads = whole waves: every lane of it is here)
    const Q80Lane c = q80_quant_group32(acc * (1.0f / L));
    zq[((int64_t)b * n_heads0 + h0) * hd + i] = (int8_t)c.qf;
    const float bsum = group32_reduce_sum(c.qf);
    if ((i & 31) == 0) {
        const int blk = (h0 * hd + i) / QB;
        zs[(int64_t)b * (n_heads0 * hd / QB) + blk] = c.d;
        zbs[(int64_t)b * (n_heads0 * hd / QB) + blk] = bsum;
    }
}
#undef ATTN_WIDE_ROWS

// GQA-grouped split variant: one workgroup owns ALL kv_mul query heads of
// a kv head (wave w = query head kvh*kv_mul+w), so the K/V rows stream
// through one CU's L1 once instead of kv_mul times through different XCD
// L2s (4x HBM amplification for 8B's 32q/8kv at long context). Waves are
// independent heads — no cross-wave merge; each writes its split partial
// directly. The model scales S by kv_mul to keep the grid full.
template <int VEC, typename KVT>
__global__ void k_attn_split_gqa(const float *__restrict__ q, int q_ld,
                                 const KVT *__restrict__ kc,
                                 const KVT *__restrict__ vc,
                                 const int *__restrict__ pos,
                                 int n_heads0, int kv_mul, int kv_dim0,
                                 float scale,
                                 float *__restrict__ ml_scratch,
                                 float *__restrict__ o_scratch) {
    const int kvh = blockIdx.x;
    const int b = blockIdx.y;
    const int sp = blockIdx.z;
    const int S = gridDim.z;
    const int hd = VEC * WAVE;
    const int plen = pos[0] + b + 1;
    const int wave = threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    const int h0 = kvh * kv_mul + wave;
    const int kv_off = kvh * hd;
    const int VEC16 = VEC * 4;
    const int lane16 = lane & 15;
    const int group = lane >> 4;

    float qreg[VEC16];
    #pragma unroll
    for (int v = 0; v < VEC16; v++)
        qreg[v] = q[(int64_t)b * q_ld + h0 * hd + lane16 * VEC16 + v] * scale;

    float m = -1e30f, l = 0.0f, o[VEC];
    #pragma unroll
    for (int v = 0; v < VEC; v++) o[v] = 0.0f;

    // 16 consecutive timesteps per round (4 group-chunks x 4 unrolled);
    // all waves walk the same rounds, so the wg's K/V reads coalesce in L1
    for (int tb0 = sp * 16; tb0 < plen; tb0 += 16 * S) {
        float su[4];
        #pragma unroll
        for (int u = 0; u < 4; u++) {
            const int tg = tb0 + u * 4 + group;
            float partial = 0.0f;
            if (tg < plen) {
                const KVT *krow = kc + (int64_t)tg * kv_dim0 + kv_off + lane16 * VEC16;
                #pragma unroll
                for (int v = 0; v < VEC16; v++)
                    partial = fmaf(qreg[v], kv_f(krow[v]), partial);
            }
            su[u] = group16_reduce_sum(partial);
        }
        float s16[16];
        float mn = m;
        #pragma unroll
        for (int u = 0; u < 4; u++) {
            #pragma unroll
            for (int gg = 0; gg < 4; gg++) {
                float v = __shfl(su[u], gg * 16, WAVE);
                if (tb0 + u * 4 + gg >= plen) v = -1e30f;
                s16[4 * u + gg] = v;
                mn = fmaxf(mn, v);
            }
        }
        const float f = __expf(m - mn);
        float w16[16];
        float lsum = 0.0f;
        #pragma unroll
        for (int i = 0; i < 16; i++) {
            w16[i] = __expf(s16[i] - mn);
            lsum += w16[i];
        }
        l = l * f + lsum;
        #pragma unroll
        for (int v = 0; v < VEC; v++) o[v] *= f;
        #pragma unroll
        for (int u = 0; u < 4; u++) {
            #pragma unroll
            for (int gg = 0; gg < 4; gg++) {
                const int t = tb0 + u * 4 + gg;
                if (t >= plen) continue;
                const KVT *vrow = vc + (int64_t)t * kv_dim0 + kv_off + lane * VEC;
                #pragma unroll
                for (int v = 0; v < VEC; v++)
                    o[v] = fmaf(w16[4 * u + gg], kv_f(vrow[v]), o[v]);
            }
        }
        m = mn;
    }

    const int64_t slot = ((int64_t)b * n_heads0 + h0) * S + sp;
    if (lane == 0) {
        ml_scratch[slot * 2] = m;
        ml_scratch[slot * 2 + 1] = l;
    }
    #pragma unroll
    for (int v = 0; v < VEC; v++)
        o_scratch[slot * hd + lane * VEC + v] = o[v];
}

// Stage 2: combine the S split partials. QUANT=true additionally emits the
// Q80 triple of the attention output directly (each workgroup owns a whole
// head = hd/32 quant blocks), eliminating the separate cast kernel the
// reference runs before the wo matmul. (A fused last-block-combine variant
// measured 2x SLOWER: per-workgroup threadfence + tail serialization.)
template <int VEC, bool QUANT>
__global__ void k_attn_combine(const float *__restrict__ ml_scratch,
                               const float *__restrict__ o_scratch,
                               float *__restrict__ y,
                               int8_t *__restrict__ zq,
                               float *__restrict__ zs,
                               float *__restrict__ zbs,
                               int n_heads0, int S) {
    const int h0 = blockIdx.x;
    const int b = blockIdx.y;
    const int hd = VEC * WAVE;  // blockDim.x == hd
    const int64_t base = ((int64_t)b * n_heads0 + h0) * S;
    float M = -1e30f;
    for (int sp = 0; sp < S; sp++)
        M = fmaxf(M, ml_scratch[(base + sp) * 2]);
    float L = 0.0f;
    for (int sp = 0; sp < S; sp++)
        L += ml_scratch[(base + sp) * 2 + 1] * __expf(ml_scratch[(base + sp) * 2] - M);
    const float invL = 1.0f / L;
    const int i = threadIdx.x;
    float acc = 0.0f;
    for (int sp = 0; sp < S; sp++)
        acc += o_scratch[(base + sp) * hd + i]
             * __expf(ml_scratch[(base + sp) * 2] - M);
    const float v = acc * invL;
    if (!QUANT) {
        y[((int64_t)b * n_heads0 + h0) * hd + i] = v;
    } else {
        const Q80Lane c = q80_quant_group32(v);
        zq[((int64_t)b * n_heads0 + h0) * hd + i] = (int8_t)c.qf;
        const float bsum = group32_reduce_sum(c.qf);
        if ((i & 31) == 0) {
            const int blk = (h0 * hd + i) / QB;
            zs[(int64_t)b * (n_heads0 * hd / QB) + blk] = c.d;
            zbs[(int64_t)b * (n_heads0 * hd / QB) + blk] = bsum;
        }
    }
}

// ------------------------------------------------------------------ rope
// style 0 = llama interleaved pairs (reference ropeLlama_F32,
// nn-cpu-ops.cpp:843-863), style 1 = falcon/neox half-rotated
// (ropeFalcon_F32, :865-885). cache [seq, hd/2, 2] = (cos, sin).
// x [B, dim0]; row b uses position pos[0]+b.
template <int STYLE>
__global__ void k_rope(float *__restrict__ x,
                       const float *__restrict__ cache,
                       const int *__restrict__ pos,
                       int dim0, int hd) {
    const int b = blockIdx.y;
    const int p = pos[0] + b;
    const int half = hd >> 1;
    float *row = x + (int64_t)b * dim0;
    const float *pc = cache + (int64_t)p * hd;  // hd floats = hd/2 pairs
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < dim0 / 2;
         i += gridDim.x * blockDim.x) {
        const int head = i / half;
        const int j = i % half;  // cache pair index
        int i0, i1;
        if (STYLE == 0) {          // pair (2j, 2j+1) within each head
            i0 = head * hd + 2 * j;
            i1 = i0 + 1;
        } else {                   // pair (j, j+hd/2) within each head
            i0 = head * hd + j;
            i1 = i0 + half;
        }
        const float cr = pc[2 * j];
        const float ci = pc[2 * j + 1];
        const float v0 = row[i0];
        const float v1 = row[i1];
        row[i0] = v0 * cr - v1 * ci;
        row[i1] = v0 * ci + v1 * cr;
    }
}

// ------------------------------------------- fused rope(q,k) + kv append
// Operates directly on the fused QKV GEMV output buffer ([B, ld] with
// q | k | v packed per row): rotates q in place, rotates k and writes it to
// the cache row pos+b, and copies v to the cache — one launch replacing
// rope(q), rope(k), kv_append (reference runs 4 separate ops here,
// llm.cpp:300-330).
template <int STYLE, typename KVT, typename ROWS = SeqRows>
__global__ void k_rope_kv(float *__restrict__ qkv, int ld,
                          int q_dim0, int kv_dim0,
                          const float *__restrict__ cache,
                          const ROWS rows,
                          KVT *__restrict__ kc,
                          KVT *__restrict__ vc,
                          int hd) {
    const int b = blockIdx.y;
    const int rp = rows.position(b);          // rope position
    const int64_t p = rows.cache_row(b, rp);  // cache row written
    const int half = hd >> 1;
    const float *pc = cache + (int64_t)rp * hd;
    float *qrow = qkv + (int64_t)b * ld;
    float *krow = qrow + q_dim0;
    const float *vrow = krow + kv_dim0;
    const int qp = q_dim0 >> 1, kp = kv_dim0 >> 1, vq = kv_dim0 >> 2;
    const int total = qp + kp + vq;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += gridDim.x * blockDim.x) {
        if (i < qp + kp) {
            const bool is_q = i < qp;
            const int ii = is_q ? i : i - qp;
            const int head = ii / half;
            const int j = ii % half;
            int i0, i1;
            if (STYLE == 0) { i0 = head * hd + 2 * j; i1 = i0 + 1; }
            else            { i0 = head * hd + j;     i1 = i0 + half; }
            const float cr = pc[2 * j];
            const float ci = pc[2 * j + 1];
            float *src = is_q ? qrow : krow;
            const float v0 = src[i0];
            const float v1 = src[i1];
            const float o0 = v0 * cr - v1 * ci;
            const float o1 = v0 * ci + v1 * cr;
            if (is_q) { src[i0] = o0; src[i1] = o1; }
            else {
                KVT *dst = kc + p * kv_dim0;
                dst[i0] = kv_c<KVT>(o0); dst[i1] = kv_c<KVT>(o1);
            }
        } else {
            const int j = (i - qp - kp) * 4;
            const float4 vv = *reinterpret_cast<const float4 *>(vrow + j);
            KVT *dst = vc + p * kv_dim0 + j;
            dst[0] = kv_c<KVT>(vv.x); dst[1] = kv_c<KVT>(vv.y);
            dst[2] = kv_c<KVT>(vv.z); dst[3] = kv_c<KVT>(vv.w);
        }
    }
}

// ------------------------------------------------------------------ kv append
// copy k,v batch rows into the caches at row pos[0]+b (reference OP_SHIFT,
// nn-cpu-ops.cpp:1419-1441).
template <typename KVT>
__global__ void k_kv_append(const float *__restrict__ k,
                            const float *__restrict__ v,
                            KVT *__restrict__ kc,
                            KVT *__restrict__ vc,
                            const int *__restrict__ pos,
                            int kv_dim0) {
    const int b = blockIdx.y;
    const int p = pos[0] + b;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < kv_dim0;
         i += gridDim.x * blockDim.x) {
        kc[(int64_t)p * kv_dim0 + i] = kv_c<KVT>(k[(int64_t)b * kv_dim0 + i]);
        vc[(int64_t)p * kv_dim0 + i] = kv_c<KVT>(v[(int64_t)b * kv_dim0 + i]);
    }
}

// Qwen3 attention prologue in one launch: per-head rmsnorm of the q/k heads
// (reference OP_RMS_NORM nColumns mode, llm.cpp:178-187) + neox rope + KV
// cache write (reference rope + shift ops). One workgroup (1 wave) per head:
// q heads normalize+rotate in place, k heads normalize+rotate into the
// cache, v heads copy to the cache.
template <typename KVT, typename ROWS = SeqRows>
__global__ void k_rope_kv_qknorm(float *__restrict__ qkv, int ld,
                                 int q_dim0, int kv_dim0,
                                 const float *__restrict__ cache,
                                 const ROWS rows,
                                 KVT *__restrict__ kc, KVT *__restrict__ vc,
                                 int hd,
                                 const float *__restrict__ wq,
                                 const float *__restrict__ wk, float eps) {
    const int b = blockIdx.y;
    const int rp = rows.position(b);          // rope position
    const int64_t p = rows.cache_row(b, rp);  // cache row written
    const int h = blockIdx.x;
    const int qh = q_dim0 / hd, kvh = kv_dim0 / hd;
    const int half = hd >> 1;
    const float *pc = cache + (int64_t)rp * hd;
    const int lane = threadIdx.x;  // blockDim == 64
    if (h >= qh + kvh) {
        // v head: plain copy into the cache
        const int hv = h - qh - kvh;
        const float *src = qkv + (int64_t)b * ld + q_dim0 + kv_dim0 + hv * hd;
        KVT *dst = vc + p * kv_dim0 + hv * hd;
        for (int i = lane; i < hd; i += WAVE) dst[i] = kv_c<KVT>(src[i]);
        return;
    }
    const bool is_q = h < qh;
    float *row = qkv + (int64_t)b * ld + (is_q ? h * hd
                                               : q_dim0 + (h - qh) * hd);
    const float *w = is_q ? wq : wk;
    float acc = 0.0f;
    for (int i = lane; i < hd; i += WAVE) {
        const float v = row[i];
        acc += v * v;
    }
    acc = wave_reduce_sum(acc);
    const float inv = rsqrtf(acc / hd + eps);
    for (int j = lane; j < half; j += WAVE) {
        const float v0 = row[j] * inv * w[j];
        const float v1 = row[j + half] * inv * w[j + half];
        const float cr = pc[2 * j], ci = pc[2 * j + 1];
        const float o0 = v0 * cr - v1 * ci;
        const float o1 = v0 * ci + v1 * cr;
        if (is_q) {
            row[j] = o0;
            row[j + half] = o1;
        } else {
            KVT *dst = kc + p * kv_dim0 + (h - qh) * hd;
            dst[j] = kv_c<KVT>(o0);
            dst[j + half] = kv_c<KVT>(o1);
        }
    }
}

// The Q80-cache form of k_rope_kv (MODE 0 = llama pairs, 1 = neox halves) and
// of k_rope_kv_qknorm (MODE 2), all in the qknorm kernel's shape: one wave per
// head, grid (q_heads + 2*kv_heads, B), hd = VEC*64. A block's 32 elements
// then sit in adjacent lanes of the wave, so its absmax is a shuffle
// reduction: a 32-lane group for a V head (lane holds elements lane + 64*i)
// and for the neox halves (lane j holds j and j + hd/2), a 16-lane group for
// the llama pairs (lane j holds 2j and 2j+1). K is quantised after the norm
// and the rope, V as the matmul left it. q is rotated in place with the
// arithmetic of the f16/f32 kernels: its bits are theirs. hd = 64 uses lanes
// 0..31 of a q/k head; the others carry zeros through the reductions and
// store nothing.
template <int MODE, int VEC, typename ROWS>
__global__ void k_rope_kv_q80(float *__restrict__ qkv, int ld,
                              int q_dim0, int kv_dim0,
                              const float *__restrict__ cache,
                              const ROWS rows,
                              int8_t *__restrict__ kc, int8_t *__restrict__ vc,
                              __half *__restrict__ ks, __half *__restrict__ vs,
                              const float *__restrict__ wq,
                              const float *__restrict__ wk, float eps) {
    constexpr int hd = VEC * WAVE;
    constexpr int half = hd >> 1;
    const int b = blockIdx.y;
    const int rp = rows.position(b);          // rope position
    const int64_t p = rows.cache_row(b, rp);  // cache row written
    const int h = blockIdx.x;
    const int qh = q_dim0 / hd, kvh = kv_dim0 / hd;
    const int nblk = kv_dim0 / QB;  // scales per cache row
    const float *pc = cache + (int64_t)rp * hd;
    const int lane = threadIdx.x;  // blockDim == 64
    if (h >= qh + kvh) {
        const int hv = h - qh - kvh;
        const float *src = qkv + (int64_t)b * ld + q_dim0 + kv_dim0 + hv * hd;
        int8_t *dst = vc + p * kv_dim0 + hv * hd;
        __half *sdst = vs + p * nblk + hv * (hd / QB);
        #pragma unroll
        for (int i = 0; i < VEC; i++) {
            const int e = lane + i * WAVE;
            const Q80Lane c = q80_quant_group32(src[e]);
            dst[e] = (int8_t)c.qf;
            if ((lane & 31) == 0) sdst[e / QB] = __float2half(c.d);
        }
        return;
    }
    const bool is_q = h < qh;
    float *row = qkv + (int64_t)b * ld + (is_q ? h * hd
                                               : q_dim0 + (h - qh) * hd);
    [[maybe_unused]] float inv = 1.0f;
    [[maybe_unused]] const float *w = is_q ? wq : wk;
    if constexpr (MODE == 2) {
        float acc = 0.0f;
        for (int i = lane; i < hd; i += WAVE) {
            const float v = row[i];
            acc += v * v;
        }
        acc = wave_reduce_sum(acc);
        inv = rsqrtf(acc / hd + eps);
    }
    const bool act = lane < half;
    const int j = act ? lane : 0;  // cache pair index
    const int i0 = MODE == 0 ? 2 * j : j;
    const int i1 = MODE == 0 ? i0 + 1 : j + half;
    float v0, v1;
    if constexpr (MODE == 2) {
        v0 = row[i0] * inv * w[i0];
        v1 = row[i1] * inv * w[i1];
    } else {
        v0 = row[i0];
        v1 = row[i1];
    }
    const float cr = pc[2 * j], ci = pc[2 * j + 1];
    // v0*cr - v1*ci and v0*ci + v1*cr as k_rope_kv and k_rope_kv_qknorm
    // contract them, spelled out: which product of the sum is rounded on its
    // own differs between those two kernels (read in their ISA), the plain
    // expressions here were paired yet another way, and q moved by an ulp
    float o0 = fmaf(v0, cr, -(v1 * ci));
    float o1 = MODE == 2 ? fmaf(v1, cr, v0 * ci) : fmaf(v0, ci, v1 * cr);
    if (is_q) {
        if (act) {
            row[i0] = o0;
            row[i1] = o1;
        }
        return;
    }
    if (!act) o0 = o1 = 0.0f;
    int8_t *dst = kc + p * kv_dim0 + (h - qh) * hd;
    __half *sdst = ks + p * nblk + (h - qh) * (hd / QB);
    if constexpr (MODE == 0) {
        const Q80Pair c = q80_quant_group16x2(o0, o1);
        if (act) {
            dst[i0] = (int8_t)c.qf0;
            dst[i1] = (int8_t)c.qf1;
            if ((lane & 15) == 0) sdst[i0 / QB] = __float2half(c.d);
        }
    } else {
        const Q80Lane c0 = q80_quant_group32(o0);
        const Q80Lane c1 = q80_quant_group32(o1);
        if (act) {
            dst[i0] = (int8_t)c0.qf;
            dst[i1] = (int8_t)c1.qf;
            if ((lane & 31) == 0) {
                sdst[i0 / QB] = __float2half(c0.d);
                sdst[i1 / QB] = __float2half(c1.d);
            }
        }
    }
}

// Row table [B, 2]: every row's pos += 1 (its cache_row_base stays).
__global__ void k_rows_advance(int *__restrict__ rows, int batch) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch) rows[2 * b + 1] += 1;
}

// ============================================================== host bindings

// f(kc, vc) with the cache pointers typed by the cache dtype: __half * (the
// default), float *, or int8_t * for the code planes of a Q80 cache. KVT
// inside f: std::remove_pointer_t<decltype(kc)>.
template <typename F>
static void with_kv_ptrs(torch::Tensor &kc, torch::Tensor &vc, F &&f) {
    TORCH_CHECK(kc.scalar_type() == vc.scalar_type(),
                "K and V caches must have one dtype");
    if (kc.scalar_type() == at::kHalf)
        f(reinterpret_cast<__half *>(kc.data_ptr<at::Half>()),
          reinterpret_cast<__half *>(vc.data_ptr<at::Half>()));
    else if (kc.scalar_type() == at::kChar)
        f(kc.data_ptr<int8_t>(), vc.data_ptr<int8_t>());
    else
        f(kc.data_ptr<float>(), vc.data_ptr<float>());
}

// The scale planes of a Q80 cache, given exactly when the caches are int8:
// float16 [rows, kv_dim0/32], contiguous, on the caches' device.
using OptTensor = c10::optional<torch::Tensor>;
struct KVScales {
    __half *k = nullptr, *v = nullptr;
};
static KVScales kv_scales(const torch::Tensor &kc, const torch::Tensor &vc,
                          const OptTensor &k_scales,
                          const OptTensor &v_scales) {
    const bool q80 = kc.scalar_type() == at::kChar
                  || vc.scalar_type() == at::kChar;
    if (!q80) {
        TORCH_CHECK(!k_scales.has_value() && !v_scales.has_value(),
                    "k_scales / v_scales go with int8 (Q80) KV caches only");
        return {};
    }
    TORCH_CHECK(k_scales.has_value() && v_scales.has_value(),
                "int8 (Q80) KV caches need k_scales= and v_scales=");
    TORCH_CHECK(kc.dim() == 2 && kc.size(1) % QB == 0 && kc.is_contiguous()
                && vc.is_contiguous() && kc.sizes() == vc.sizes(),
                "Q80 KV caches: contiguous int8 [rows, kv_dim0], kv_dim0 a "
                "multiple of 32");
    KVScales out;
    int i = 0;
    for (const torch::Tensor *s : {&*k_scales, &*v_scales}) {
        TORCH_CHECK(s->scalar_type() == at::kHalf, "KV scales must be float16");
        TORCH_CHECK(s->dim() == 2 && s->size(0) == kc.size(0)
                    && s->size(1) == kc.size(1) / QB,
                    "KV scales must be [rows, kv_dim0/32] = [", kc.size(0),
                    ", ", kc.size(1) / QB, "]");
        TORCH_CHECK(s->is_contiguous(), "KV scales must be contiguous");
        TORCH_CHECK(s->device() == kc.device(),
                    "KV scales must be on the caches' device");
        (i++ ? out.v : out.k) =
            reinterpret_cast<__half *>(s->data_ptr<at::Half>());
    }
    return out;
}

// f(VEC) with VEC = head_dim / 64 (elements per lane of the head's wave) as
// a std::integral_constant
template <typename F>
static void with_head_vec(int64_t head_dim, F &&f) {
    if (head_dim == 128) f(std::integral_constant<int, 2>{});
    else if (head_dim == 64) f(std::integral_constant<int, 1>{});
    else TORCH_CHECK(false, "unsupported head_dim ", head_dim);
}

void rope(torch::Tensor x, torch::Tensor cache, torch::Tensor pos,
          int64_t head_dim, int64_t style) {
    CHECK_CUDA(x);
    const int B = x.size(0);
    const int dim0 = x.size(1);
    const dim3 grid(ceil_div(dim0 / 2, 256), B);
    if (style == 0)
        hipLaunchKernelGGL(k_rope<0>, grid, dim3(256), 0, cur_stream(),
                           x.data_ptr<float>(), cache.data_ptr<float>(),
                           pos.data_ptr<int>(), dim0, (int)head_dim);
    else
        hipLaunchKernelGGL(k_rope<1>, grid, dim3(256), 0, cur_stream(),
                           x.data_ptr<float>(), cache.data_ptr<float>(),
                           pos.data_ptr<int>(), dim0, (int)head_dim);
}

void kv_append(torch::Tensor k, torch::Tensor v, torch::Tensor kc,
               torch::Tensor vc, torch::Tensor pos) {
    CHECK_CUDA(k);
    const int B = k.size(0);
    const int kv_dim0 = k.size(1);
    const dim3 grid(ceil_div(kv_dim0, 256), B);
    with_kv_ptrs(kc, vc, [&](auto *kcp, auto *vcp) {
        using KVT = std::remove_pointer_t<decltype(kcp)>;
        if constexpr (kKVQ80<KVT>) {
            TORCH_CHECK(false, "kv_append has no Q80 KV cache form: write an "
                        "int8 cache with rope_kv(..., k_scales=, v_scales=)");
        } else {
            hipLaunchKernelGGL(k_kv_append<KVT>, grid, dim3(256), 0,
                               cur_stream(), k.data_ptr<float>(),
                               v.data_ptr<float>(), kcp, vcp,
                               pos.data_ptr<int>(), kv_dim0);
        }
    });
}

// A row table as the kernels read it: int32 [>= batch, 2], contiguous, on
// the device. Its contents (slot bases and positions inside the caches) are
// the caller's to validate: the host never sees them in a captured step.
static TableRows table_rows(const torch::Tensor &rows, int64_t batch) {
    CHECK_CUDA(rows);
    TORCH_CHECK(rows.scalar_type() == at::kInt && rows.dim() == 2
                && rows.size(1) == 2 && rows.is_contiguous()
                && rows.size(0) >= batch,
                "row table must be a contiguous int32 [>= batch, 2]");
    return TableRows{rows.data_ptr<int>()};
}

// The paged form of a row table: word 0 of a row indexes page_table (int32
// [n_slots, pages_per_seq], contiguous, on the cache's device), whose
// entries are page ids of a cache of whole pages of page_size rows. The
// contents of both tables are the caller's to validate.
static PagedRows paged_rows(const torch::Tensor &rows,
                            const torch::Tensor &page_table, int64_t page_size,
                            int64_t batch, const torch::Tensor &kc) {
    const TableRows t = table_rows(rows, batch);
    CHECK_CUDA(page_table);
    TORCH_CHECK(page_table.scalar_type() == at::kInt && page_table.dim() == 2
                && page_table.is_contiguous() && page_table.numel() > 0
                && page_table.device() == kc.device()
                && rows.device() == kc.device(),
                "page table must be a contiguous int32 [n_slots, "
                "pages_per_seq] on the cache's device");
    TORCH_CHECK(page_size >= 4 && page_size <= 256
                && (page_size & (page_size - 1)) == 0,
                "page_size must be a power of two in 4..256 (got ",
                page_size, ")");
    TORCH_CHECK(kc.size(0) % page_size == 0,
                "a paged cache holds whole pages: ", kc.size(0),
                " rows, page_size ", page_size);
    int shift = 0;
    while ((int64_t(1) << shift) < page_size) shift++;
    return PagedRows{t.rows, page_table.data_ptr<int>(), shift};
}

// The launches of attention, for any row addressing: the wide single kernel
// when splits == 1 and the output is the Q80 triple, else split + combine.
// The GQA-grouped experiment exists for the single-sequence form only.
template <typename ROWS>
static void attn_launch(torch::Tensor &q, int64_t q_ld, torch::Tensor &kc,
                        torch::Tensor &vc, torch::Tensor &y, ROWS rows,
                        int64_t batch, int64_t n_heads0, int64_t kv_mul,
                        int64_t head_dim, int64_t splits,
                        torch::Tensor &ml_scratch, torch::Tensor &o_scratch,
                        c10::optional<torch::Tensor> &zq,
                        c10::optional<torch::Tensor> &zs,
                        c10::optional<torch::Tensor> &zbs,
                        const OptTensor &k_scales, const OptTensor &v_scales) {
    CHECK_CUDA(q);
    const KVScales sc = kv_scales(kc, vc, k_scales, v_scales);
    const int kv_dim0 = kc.size(1);
    const float scale = 1.0f / sqrtf((float)head_dim);
    const dim3 grid(n_heads0, batch, splits);
    const dim3 cgrid(n_heads0, batch);
    const bool quant = zq.has_value();
    // quant: the Q80 triple is the output, y is not written (and vice versa)
    float *yp = quant ? nullptr : y.data_ptr<float>();
    int8_t *zqp = quant ? zq->data_ptr<int8_t>() : nullptr;
    float *zsp = quant ? zs->data_ptr<float>() : nullptr;
    float *zbsp = quant ? zbs->data_ptr<float>() : nullptr;
    // GQA grouping experiment: one wg per (kv head, split) with kv_mul
    // waves sharing the K/V stream through L1. Measured ~20% SLOWER
    // end-to-end (448 vs 545 tok/s short-ctx 8B; MoE 366->255) — the L2
    // already absorbs the GQA re-reads and the grown combine fan-in costs
    // more than the saved traffic. Kept behind DLLAMA_GQA_ATTN=1.
    static const bool env_gqa =
        std::getenv("DLLAMA_GQA_ATTN") && atoi(std::getenv("DLLAMA_GQA_ATTN")) == 1;
    const bool gqa = std::is_same_v<ROWS, SeqRows> && env_gqa && kv_mul > 1
        && kv_mul <= 8 && n_heads0 % kv_mul == 0 && splits > 1;
    // splits==1 + quant output: the wide kernel normalizes and emits the Q80
    // triple itself, no scratch and no combine launch
    const bool wide = splits == 1 && quant;
    with_head_vec(head_dim, [&](auto vec_const) {
        constexpr int V = decltype(vec_const)::value;
        with_kv_ptrs(kc, vc, [&](auto *kcp, auto *vcp) {
            using KVT = std::remove_pointer_t<decltype(kcp)>;
            if constexpr (kKVQ80<KVT>) {
                TORCH_CHECK(!env_gqa, "the DLLAMA_GQA_ATTN experiment has no Q80 "
                            "KV cache form: unset it");
                using QROWS = Q80Rows<ROWS>;
                const QROWS qrows{rows, sc.k, sc.v};
                if (wide)
                    hipLaunchKernelGGL((k_attn_wide<V, KVT, QROWS>), cgrid,
                                       dim3(1024), 0, cur_stream(),
                                       q.data_ptr<float>(), (int)q_ld, kcp,
                                       vcp, qrows, (int)n_heads0,
                                       (int)kv_mul, kv_dim0, scale, zqp, zsp,
                                       zbsp);
                else
                    hipLaunchKernelGGL((k_attn_split<V, KVT, QROWS>), grid,
                                       dim3(256), 0, cur_stream(),
                                       q.data_ptr<float>(), (int)q_ld, kcp,
                                       vcp, qrows, (int)n_heads0,
                                       (int)kv_mul, kv_dim0, scale,
                                       ml_scratch.data_ptr<float>(),
                                       o_scratch.data_ptr<float>());
                return;
            } else {
                if (wide) {
                    hipLaunchKernelGGL((k_attn_wide<V, KVT, ROWS>), cgrid,
                                       dim3(1024), 0, cur_stream(),
                                       q.data_ptr<float>(), (int)q_ld, kcp, vcp,
                                       rows, (int)n_heads0, (int)kv_mul, kv_dim0,
                                       scale, zqp, zsp, zbsp);
                    return;
                }
                if constexpr (std::is_same_v<ROWS, SeqRows>) {
                    if (gqa) {
                        hipLaunchKernelGGL((k_attn_split_gqa<V, KVT>),
                                           dim3(n_heads0 / kv_mul, batch, splits),
                                           dim3(kv_mul * WAVE), 0,
                                           cur_stream(), q.data_ptr<float>(), (int)q_ld,
                                           kcp, vcp, rows.pos, (int)n_heads0,
                                           (int)kv_mul, kv_dim0, scale,
                                           ml_scratch.data_ptr<float>(),
                                           o_scratch.data_ptr<float>());
                        return;
                    }
                }
                hipLaunchKernelGGL((k_attn_split<V, KVT, ROWS>), grid, dim3(256),
                                   0, cur_stream(), q.data_ptr<float>(), (int)q_ld,
                                   kcp, vcp, rows,
                                   (int)n_heads0, (int)kv_mul, kv_dim0, scale,
                                   ml_scratch.data_ptr<float>(),
                                   o_scratch.data_ptr<float>());
            }
        });
        if (wide) return;
        auto combine = [&](auto quant_const) {
            hipLaunchKernelGGL((k_attn_combine<V, decltype(quant_const)::value>),
                               cgrid, dim3(V * WAVE), 0, cur_stream(),
                               ml_scratch.data_ptr<float>(),
                               o_scratch.data_ptr<float>(), yp, zqp, zsp, zbsp,
                               (int)n_heads0, (int)splits);
        };
        if (quant) combine(std::true_type{});
        else combine(std::false_type{});
    });
}

void attn(torch::Tensor q, int64_t q_ld, torch::Tensor kc, torch::Tensor vc,
          torch::Tensor y, torch::Tensor pos, int64_t batch, int64_t n_heads0,
          int64_t kv_mul, int64_t head_dim, int64_t splits,
          torch::Tensor ml_scratch, torch::Tensor o_scratch,
          torch::Tensor /*counter: unused, kept for the binding signature*/,
          c10::optional<torch::Tensor> zq = c10::nullopt,
          c10::optional<torch::Tensor> zs = c10::nullopt,
          c10::optional<torch::Tensor> zbs = c10::nullopt,
                OptTensor k_scales = c10::nullopt,
                OptTensor v_scales = c10::nullopt) {
    attn_launch(q, q_ld, kc, vc, y, SeqRows{pos.data_ptr<int>()}, batch,
                n_heads0, kv_mul, head_dim, splits, ml_scratch, o_scratch,
                zq, zs, zbs,
                k_scales, v_scales);
}

// Row b attends over cache rows base_b .. base_b+pos_b of the row table.
void attn_rows(torch::Tensor q, int64_t q_ld, torch::Tensor kc, torch::Tensor vc,
               torch::Tensor y, torch::Tensor rows, int64_t batch,
               int64_t n_heads0, int64_t kv_mul, int64_t head_dim,
               int64_t splits, torch::Tensor ml_scratch, torch::Tensor o_scratch,
               c10::optional<torch::Tensor> zq = c10::nullopt,
               c10::optional<torch::Tensor> zs = c10::nullopt,
               c10::optional<torch::Tensor> zbs = c10::nullopt,
                OptTensor k_scales = c10::nullopt,
                OptTensor v_scales = c10::nullopt) {
    attn_launch(q, q_ld, kc, vc, y, table_rows(rows, batch), batch, n_heads0,
                kv_mul, head_dim, splits, ml_scratch, o_scratch, zq, zs, zbs,
                k_scales, v_scales);
}

// attn_rows over a paged cache: row b attends over positions 0..pos_b of its
// sequence, each found through the page table.
void attn_paged(torch::Tensor q, int64_t q_ld, torch::Tensor kc, torch::Tensor vc,
                torch::Tensor y, torch::Tensor rows, torch::Tensor page_table,
                int64_t page_size, int64_t batch, int64_t n_heads0,
                int64_t kv_mul, int64_t head_dim, int64_t splits,
                torch::Tensor ml_scratch, torch::Tensor o_scratch,
                c10::optional<torch::Tensor> zq = c10::nullopt,
                c10::optional<torch::Tensor> zs = c10::nullopt,
                c10::optional<torch::Tensor> zbs = c10::nullopt,
                OptTensor k_scales = c10::nullopt,
                OptTensor v_scales = c10::nullopt) {
    attn_launch(q, q_ld, kc, vc, y,
                paged_rows(rows, page_table, page_size, batch, kc), batch,
                n_heads0, kv_mul, head_dim, splits, ml_scratch, o_scratch,
                zq, zs, zbs,
                k_scales, v_scales);
}

// The Q80 write kernel for either launcher below; mode as k_rope_kv_q80's
// MODE (0/1 = the rope style, 2 = q/k-norm + neox).
template <typename ROWS>
static void rope_kv_q80_launch(int mode, torch::Tensor &qkv, int64_t ld,
                               int64_t q_dim0, int64_t kv_dim0,
                               torch::Tensor &cache, ROWS rows,
                               torch::Tensor &kc, int8_t *kcp, int8_t *vcp,
                               const KVScales &sc, int64_t head_dim,
                               const float *wq, const float *wk, float eps,
                               int64_t batch) {
    TORCH_CHECK(kc.size(1) == kv_dim0 && q_dim0 % head_dim == 0
                && kv_dim0 % head_dim == 0,
                "Q80 KV write: q_dim0 and kv_dim0 are whole heads and "
                "kv_dim0 is the cache's row width");
    const dim3 grid((q_dim0 + 2 * kv_dim0) / head_dim, batch);
    with_head_vec(head_dim, [&](auto vec_const) {
        constexpr int V = decltype(vec_const)::value;
        auto *kern = mode == 0 ? k_rope_kv_q80<0, V, ROWS>
                   : mode == 1 ? k_rope_kv_q80<1, V, ROWS>
                               : k_rope_kv_q80<2, V, ROWS>;
        hipLaunchKernelGGL(kern, grid, dim3(WAVE), 0, cur_stream(),
                           qkv.data_ptr<float>(), (int)ld, (int)q_dim0,
                           (int)kv_dim0, cache.data_ptr<float>(), rows, kcp,
                           vcp, sc.k, sc.v, wq, wk, eps);
    });
}

template <typename ROWS>
static void rope_kv_launch(torch::Tensor &qkv, int64_t ld, int64_t q_dim0,
                           int64_t kv_dim0, torch::Tensor &cache, ROWS rows,
                           torch::Tensor &kc, torch::Tensor &vc,
                           int64_t head_dim, int64_t style, int64_t batch,
                           const OptTensor &k_scales,
                           const OptTensor &v_scales) {
    CHECK_CUDA(qkv);
    const KVScales sc = kv_scales(kc, vc, k_scales, v_scales);
    const int total = (int)(q_dim0 / 2 + kv_dim0 / 2 + kv_dim0 / 4);
    const dim3 grid(ceil_div(total, 256), batch);
    with_kv_ptrs(kc, vc, [&](auto *kcp, auto *vcp) {
        using KVT = std::remove_pointer_t<decltype(kcp)>;
        if constexpr (kKVQ80<KVT>) {
            rope_kv_q80_launch(style == 0 ? 0 : 1, qkv, ld, q_dim0, kv_dim0,
                               cache, rows, kc, kcp, vcp, sc, head_dim,
                               nullptr, nullptr, 0.0f, batch);
        } else {
            auto *kern = style == 0 ? k_rope_kv<0, KVT, ROWS>
                                    : k_rope_kv<1, KVT, ROWS>;
            hipLaunchKernelGGL(kern, grid, dim3(256), 0, cur_stream(),
                               qkv.data_ptr<float>(), (int)ld, (int)q_dim0,
                               (int)kv_dim0, cache.data_ptr<float>(), rows,
                               kcp, vcp, (int)head_dim);
        }
    });
}

void rope_kv(torch::Tensor qkv, int64_t ld, int64_t q_dim0, int64_t kv_dim0,
             torch::Tensor cache, torch::Tensor pos, torch::Tensor kc,
             torch::Tensor vc, int64_t head_dim, int64_t style, int64_t batch,
             OptTensor k_scales = c10::nullopt,
             OptTensor v_scales = c10::nullopt) {
    rope_kv_launch(qkv, ld, q_dim0, kv_dim0, cache,
                   SeqRows{pos.data_ptr<int>()}, kc, vc, head_dim, style, batch,
                   k_scales, v_scales);
}

void rope_kv_rows(torch::Tensor qkv, int64_t ld, int64_t q_dim0, int64_t kv_dim0,
                  torch::Tensor cache, torch::Tensor rows, torch::Tensor kc,
                  torch::Tensor vc, int64_t head_dim, int64_t style,
                  int64_t batch, OptTensor k_scales = c10::nullopt,
                  OptTensor v_scales = c10::nullopt) {
    rope_kv_launch(qkv, ld, q_dim0, kv_dim0, cache, table_rows(rows, batch),
                   kc, vc, head_dim, style, batch, k_scales, v_scales);
}

void rope_kv_paged(torch::Tensor qkv, int64_t ld, int64_t q_dim0, int64_t kv_dim0,
                   torch::Tensor cache, torch::Tensor rows,
                   torch::Tensor page_table, int64_t page_size,
                   torch::Tensor kc, torch::Tensor vc, int64_t head_dim,
                   int64_t style, int64_t batch,
                   OptTensor k_scales = c10::nullopt,
                   OptTensor v_scales = c10::nullopt) {
    rope_kv_launch(qkv, ld, q_dim0, kv_dim0, cache,
                   paged_rows(rows, page_table, page_size, batch, kc), kc, vc,
                   head_dim, style, batch, k_scales, v_scales);
}

template <typename ROWS>
static void rope_kv_qknorm_launch(torch::Tensor &qkv, int64_t ld, int64_t q_dim0,
                                  int64_t kv_dim0, torch::Tensor &cache,
                                  ROWS rows, torch::Tensor &kc,
                                  torch::Tensor &vc, int64_t head_dim,
                                  torch::Tensor &wq, torch::Tensor &wk,
                                  double eps, int64_t batch,
                                  const OptTensor &k_scales,
                                  const OptTensor &v_scales) {
    CHECK_CUDA(qkv);
    const KVScales sc = kv_scales(kc, vc, k_scales, v_scales);
    const int heads = (int)((q_dim0 + 2 * kv_dim0) / head_dim);
    const dim3 grid(heads, batch);
    with_kv_ptrs(kc, vc, [&](auto *kcp, auto *vcp) {
        using KVT = std::remove_pointer_t<decltype(kcp)>;
        if constexpr (kKVQ80<KVT>) {
            rope_kv_q80_launch(2, qkv, ld, q_dim0, kv_dim0, cache, rows, kc,
                               kcp, vcp, sc, head_dim, wq.data_ptr<float>(),
                               wk.data_ptr<float>(), (float)eps, batch);
        } else {
            hipLaunchKernelGGL((k_rope_kv_qknorm<KVT, ROWS>), grid, dim3(WAVE),
                               0, cur_stream(), qkv.data_ptr<float>(), (int)ld,
                               (int)q_dim0, (int)kv_dim0,
                               cache.data_ptr<float>(), rows, kcp, vcp,
                               (int)head_dim, wq.data_ptr<float>(),
                               wk.data_ptr<float>(), (float)eps);
        }
    });
}

void rope_kv_qknorm(torch::Tensor qkv, int64_t ld, int64_t q_dim0,
                    int64_t kv_dim0, torch::Tensor cache, torch::Tensor pos,
                    torch::Tensor kc, torch::Tensor vc, int64_t head_dim,
                    torch::Tensor wq, torch::Tensor wk, double eps,
                    int64_t batch, OptTensor k_scales = c10::nullopt,
                    OptTensor v_scales = c10::nullopt) {
    rope_kv_qknorm_launch(qkv, ld, q_dim0, kv_dim0, cache,
                          SeqRows{pos.data_ptr<int>()}, kc, vc, head_dim, wq,
                          wk, eps, batch, k_scales, v_scales);
}

void rope_kv_qknorm_rows(torch::Tensor qkv, int64_t ld, int64_t q_dim0,
                         int64_t kv_dim0, torch::Tensor cache,
                         torch::Tensor rows, torch::Tensor kc, torch::Tensor vc,
                         int64_t head_dim, torch::Tensor wq, torch::Tensor wk,
                         double eps, int64_t batch,
                         OptTensor k_scales = c10::nullopt,
                         OptTensor v_scales = c10::nullopt) {
    rope_kv_qknorm_launch(qkv, ld, q_dim0, kv_dim0, cache,
                          table_rows(rows, batch), kc, vc, head_dim, wq, wk,
                          eps, batch, k_scales, v_scales);
}

void rope_kv_qknorm_paged(torch::Tensor qkv, int64_t ld, int64_t q_dim0,
                          int64_t kv_dim0, torch::Tensor cache,
                          torch::Tensor rows, torch::Tensor page_table,
                          int64_t page_size, torch::Tensor kc,
                          torch::Tensor vc, int64_t head_dim, torch::Tensor wq,
                          torch::Tensor wk, double eps, int64_t batch,
                          OptTensor k_scales = c10::nullopt,
                          OptTensor v_scales = c10::nullopt) {
    rope_kv_qknorm_launch(qkv, ld, q_dim0, kv_dim0, cache,
                          paged_rows(rows, page_table, page_size, batch, kc),
                          kc, vc, head_dim, wq, wk, eps, batch, k_scales,
                          v_scales);
}

// pos += 1 in the first `batch` rows of a row table: a captured all-decode
// step advances itself, as pos_inc does for the single sequence
void rows_advance(torch::Tensor rows, int64_t batch) {
    table_rows(rows, batch);
    hipLaunchKernelGGL(k_rows_advance, dim3(ceil_div((int)batch, WAVE)),
                       dim3(WAVE), 0, cur_stream(), rows.data_ptr<int>(),
                       (int)batch);
}

// the scale planes of a Q80 cache: keyword arguments of the nine positional
// bindings, required exactly when the caches are int8
#define KV_SCALE_ARGS \
    py::arg("k_scales") = py::none(), py::arg("v_scales") = py::none()
// rope_kv* / rope_kv_qknorm*: `where` is pos, rows, or rows + the page table
#define ROPE_KV_HEAD \
    py::arg("qkv"), py::arg("ld"), py::arg("q_dim0"), py::arg("kv_dim0"), \
    py::arg("cache")
#define ROPE_KV_TAIL \
    py::arg("kc"), py::arg("vc"), py::arg("head_dim"), py::arg("style"), \
    py::arg("batch"), KV_SCALE_ARGS
#define ROPE_KV_QKNORM_TAIL \
    py::arg("kc"), py::arg("vc"), py::arg("head_dim"), py::arg("wq"), \
    py::arg("wk"), py::arg("eps"), py::arg("batch"), KV_SCALE_ARGS

void register_attn(py::module &m) {
    m.def("rope_kv_qknorm", &rope_kv_qknorm, ROPE_KV_HEAD, py::arg("pos"),
          ROPE_KV_QKNORM_TAIL);
    m.def("rope_kv_qknorm_rows", &rope_kv_qknorm_rows, ROPE_KV_HEAD,
          py::arg("rows"), ROPE_KV_QKNORM_TAIL);
    m.def("rope", &rope);
    m.def("rope_kv", &rope_kv, ROPE_KV_HEAD, py::arg("pos"), ROPE_KV_TAIL);
    m.def("rope_kv_rows", &rope_kv_rows, ROPE_KV_HEAD, py::arg("rows"),
          ROPE_KV_TAIL);
    m.def("rows_advance", &rows_advance);
    m.def("attn_rows", &attn_rows, py::arg("q"), py::arg("q_ld"), py::arg("kc"),
          py::arg("vc"), py::arg("y"), py::arg("rows"), py::arg("batch"),
          py::arg("n_heads0"), py::arg("kv_mul"), py::arg("head_dim"),
          py::arg("splits"), py::arg("ml_scratch"), py::arg("o_scratch"),
          py::arg("zq") = py::none(), py::arg("zs") = py::none(),
          py::arg("zbs") = py::none(), KV_SCALE_ARGS);
    m.def("rope_kv_paged", &rope_kv_paged, ROPE_KV_HEAD, py::arg("rows"),
          py::arg("page_table"), py::arg("page_size"), ROPE_KV_TAIL);
    m.def("rope_kv_qknorm_paged", &rope_kv_qknorm_paged, ROPE_KV_HEAD,
          py::arg("rows"), py::arg("page_table"), py::arg("page_size"),
          ROPE_KV_QKNORM_TAIL);
    m.def("attn_paged", &attn_paged, py::arg("q"), py::arg("q_ld"),
          py::arg("kc"), py::arg("vc"), py::arg("y"), py::arg("rows"),
          py::arg("page_table"), py::arg("page_size"), py::arg("batch"),
          py::arg("n_heads0"), py::arg("kv_mul"), py::arg("head_dim"),
          py::arg("splits"), py::arg("ml_scratch"), py::arg("o_scratch"),
          py::arg("zq") = py::none(), py::arg("zs") = py::none(),
          py::arg("zbs") = py::none(), KV_SCALE_ARGS);
    m.def("kv_append", &kv_append);
    m.def("attn", &attn, py::arg("q"), py::arg("q_ld"), py::arg("kc"), py::arg("vc"),
          py::arg("y"), py::arg("pos"), py::arg("batch"), py::arg("n_heads0"),
          py::arg("kv_mul"), py::arg("head_dim"), py::arg("splits"),
          py::arg("ml_scratch"), py::arg("o_scratch"), py::arg("counter"),
          py::arg("zq") = py::none(), py::arg("zs") = py::none(),
          py::arg("zbs") = py::none(), KV_SCALE_ARGS);
}
