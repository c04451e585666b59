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
// WideRows: SeqRows for a prompt chunk of more than 32 rows. The rows are
// placed as SeqRows places them; the type tells k_attn_chunk to cut the one
// sequence into runs itself: run y is rows 32y .. min(32y + 31, batch - 1).
struct WideRows {
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

// ------------------------------------------------- tiled MFMA chunk attention
// The prompt-chunk producer of the split scratch: the rows of a chunk differ
// only in their causal mask, so one workgroup serves a whole run (<= 32
// consecutive batch rows of one sequence) for all kv_mul query heads of a KV
// head, and every K/V tile is read from the cache once per workgroup instead
// of once per (head, row). Grid (n_kv_heads0, n_runs, S), 4 waves; wave w
// owns query heads w, w+4, .. of the KV head (one pass over the timesteps
// per group of 4 heads). Split sp walks the 32-timestep tiles sp, sp+S, ..
// below the run's longest row; the grid does not depend on positions.
//
// Layouts (v_mfma_f32_32x32x16_f16, verified by tools/mfma_f16_probe.hip):
// A[m][k] and B[k][n] hold k = 8*(lane>>5)+j in half j of lane (m or n)+32*hi;
// C[m][n] holds n = lane&31, m = (r&3) + 8*(r>>2) + 4*(lane>>5) in register r.
// Scores are computed transposed, S^T = K Q^T (m = timestep, n = query row):
// a lane then holds 16 scores of ONE query row, so the online softmax is
// lane-local but for one exchange with lane^32, and registers 8c..8c+7 of
// the accumulator, rounded to f16, are directly the B operand of
// O^T += V^T P^T over timesteps t = 16c + 8*(j>>2) + 4*hi + (j&3). The A
// operand V^T gathers the same timesteps (k is only summed over): V is
// transposed on its way into LDS, so that gather is two 8-byte LDS reads.
// O^T again holds the lane's query row: m, l and the rescale stay per lane.
//
// Rounding points: q*scale (f32) -> f16 once, P -> f16 per tile, and K and V
// of a Q80 cache: code * d rounded to f16; scores, m, l and O accumulate in
// f32.
//
// Forms: KVT is the cache element (__half, or int8_t for the code planes of a
// Q80 cache with ROWS = Q80Rows<..>), ROWS any of the three addressing
// policies. They differ only in how a tile gets from the cache into LDS
// (tile_load / tile_store below); LDS always holds f16 tiles and everything
// after the barrier is shared code.
typedef _Float16 v8h_t __attribute__((ext_vector_type(8)));
typedef _Float16 v4h_t __attribute__((ext_vector_type(4)));
typedef float v16f_t __attribute__((ext_vector_type(16)));

// The kernel's independent f32 multiplies and fmas (the accumulator rescale,
// the q scaling, the softmax exponents) go through mul_f32 / fma_f32
// (dllama_common.h), which keep packed f32 VALU ops out of this kernel
// (checked in its disassembly: no v_pk_*_f32).

constexpr int CHUNK_T = 32;     // timesteps per tile = MFMA M of the scores
constexpr int CHUNK_ROWS = 32;  // query rows per run = MFMA N
constexpr int CHUNK_NW = 4;     // waves per workgroup

// 8 consecutive Q80 codes (two dwords of a cache row) times their block's
// scale, as f16: f16(code) is exact and the one f16 multiply rounds the exact
// product code * d once, so this is f16(code * f32(d)).
__device__ __forceinline__ v8h_t q80_codes_f16(int2 c, _Float16 d) {
    v8h_t out;
    #pragma unroll
    for (int i = 0; i < 8; i++) {
        const int w = i < 4 ? c.x : c.y;
        out[i] = (_Float16)(short)(int8_t)(w >> (8 * (i & 3)));
    }
    return out * d;
}

// The same values for the 4 codes of one dword, without a sign extension per
// byte. code ^ 0x80 = code + 128 as an unsigned byte u; a half with the bits
// 0x6400 | u is 1024 + u exactly (exponent 2^10, u in the low mantissa bits),
// so two byte permutes build the four halves 1152 + code, one packed add of
// -1152 leaves f16(code) (an integer below 2^11: exact), and the packed
// multiply rounds code * d once as above.
__device__ __forceinline__ v4h_t q80_dword_f16(int w, _Float16 d) {
    const unsigned u = (unsigned)w ^ 0x80808080u;
    // selector bytes 0..3 take bytes of the second operand, 4 a byte 0x64
    const unsigned lo = __builtin_amdgcn_perm(0x64646464u, u, 0x04010400u);
    const unsigned hi = __builtin_amdgcn_perm(0x64646464u, u, 0x04030402u);
    typedef unsigned v2u_t __attribute__((ext_vector_type(2)));
    const v4h_t biased = __builtin_bit_cast(v4h_t, v2u_t{lo, hi});
    return (biased - (_Float16)1152.0f) * d;
}

template <int VEC, typename KVT, typename ROWS>
__global__ void __launch_bounds__(CHUNK_NW * WAVE, 2)
k_attn_chunk(const float *__restrict__ q, int q_ld,
             const KVT *__restrict__ kc_all,
             const KVT *__restrict__ vc_all,
             const ROWS rows, const int *__restrict__ runs, int batch,
             int n_heads0, int kv_mul, int kv_dim0, float scale,
             float *__restrict__ ml_scratch, float *__restrict__ o_scratch) {
    constexpr bool Q8 = kKVQ80<KVT>;
    constexpr int hd = VEC * WAVE;
    constexpr int KLD = hd + 8;       // halves per K row: 16-byte rows, 4-bank skew
    constexpr int VLD = CHUNK_T + 4;  // halves per V^T row (one d): 8-byte rows
    constexpr int DCH = hd / 8;       // 16-byte chunks per cache row of the head
    constexpr int NLD = CHUNK_T * DCH / (CHUNK_NW * WAVE);  // chunks per thread
    static_assert(NLD * CHUNK_NW * WAVE == CHUNK_T * DCH, "tile / threads");
    __shared__ __attribute__((aligned(16))) _Float16 sk[2][CHUNK_T * KLD];
    __shared__ __attribute__((aligned(16))) _Float16 sv[2][hd * VLD];

    const int kvh = blockIdx.x;
    const int sp = blockIdx.z;
    const int S = gridDim.z;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int lane = threadIdx.x % WAVE;
    const int row = lane & 31;  // query row of the run (B / C operand column)
    const int hi = lane >> 5;

    // the run: SeqRows = the whole batch; a table run is clamped to the batch
    // and to the tile, so a bad table cannot send a load or store astray
    int b0 = 0, n = batch;
    if constexpr (std::is_base_of_v<WideRows, ROWS>) {
        // the host launches ceil(batch / 32) runs: b0 < batch
        b0 = min((int)blockIdx.y * CHUNK_ROWS, batch - 1);
        n = batch - b0;
    } else if constexpr (!std::is_base_of_v<SeqRows, ROWS>) {
        b0 = min(max(runs[2 * blockIdx.y], 0), batch - 1);
        n = min(runs[2 * blockIdx.y + 1], batch - b0);
    }
    n = min(n, CHUNK_ROWS);
    const bool real = row < n;  // else a padding row: q = 0, never written
    const int b = b0 + (real ? row : 0);
    int plen = real ? rows.position(b) + 1 : 0;
    int maxlen = plen, minlen;
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        maxlen = max(maxlen, __shfl_xor(maxlen, off, WAVE));
    maxlen = __builtin_amdgcn_readfirstlane(maxlen);
    if (!real) plen = maxlen;  // a padding row masks nothing
    minlen = plen;
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        minlen = min(minlen, __shfl_xor(minlen, off, WAVE));
    minlen = __builtin_amdgcn_readfirstlane(minlen);

    const KVT *kc = kc_all + rows.cache_base(b0) * kv_dim0 + kvh * hd;
    const KVT *vc = vc_all + rows.cache_base(b0) * kv_dim0 + kvh * hd;
    // Q80: the scale planes, f16 [rows, kv_dim0/32], from the same cache row
    [[maybe_unused]] const int nblk = kv_dim0 / QB;
    [[maybe_unused]] const _Float16 *ks = nullptr, *vs = nullptr;
    if constexpr (Q8) {
        const int64_t sb = rows.cache_base(b0) * nblk + kvh * (hd / QB);
        ks = reinterpret_cast<const _Float16 *>(rows.ks) + sb;
        vs = reinterpret_cast<const _Float16 *>(rows.vs) + sb;
    }

    // staging: thread holds NLD 8-element chunks of the K tile and of the V
    // tile in registers between their global load and their LDS store: 16
    // bytes of f16, or 8 bytes of Q80 codes and their block's f16 scale,
    // which tile_store turns into the same f16 tile (code * d rounded to f16
    // once). A timestep at or past maxlen (last tile only) re-reads row
    // maxlen-1: a valid row, masked below.
    //
    // Paged: the cache row of a timestep comes from the run's page list (all
    // rows of a run are one sequence: b0's). The clamp keeps every lookup
    // below maxlen, in pages the host checked to be mapped, and inside the
    // tile, so with pages of 32 rows or more the whole tile lies in one
    // page: one workgroup-uniform id per tile. Smaller pages look up per
    // thread (the threads of a timestep share the address). page_fetch runs
    // one tile ahead of tile_load, itself one tile ahead of use: neither the
    // K/V loads nor the MFMA phase ever wait on a table lookup in flight.
    using Staged = std::conditional_t<Q8, int2, v8h_t>;
    Staged kreg[NLD], vreg[NLD];
    [[maybe_unused]] _Float16 kscl[NLD], vscl[NLD];
    [[maybe_unused]] int pgid[NLD];  // page of each chunk of the next tile_load
    [[maybe_unused]] const int *seqp = nullptr;
    if constexpr (ROWS::kPaged)
        seqp = rows.pages + __builtin_amdgcn_readfirstlane(rows.rows[2 * b0]);
    auto page_fetch = [&](int tile) {
        if constexpr (ROWS::kPaged) {
            if (tile * CHUNK_T >= maxlen) return;  // no such tile
            if (rows.shift >= 5) {
                const int id = seqp[(tile * CHUNK_T) >> rows.shift];
                #pragma unroll
                for (int it = 0; it < NLD; it++) pgid[it] = id;
            } else {
                #pragma unroll
                for (int it = 0; it < NLD; it++) {
                    const int idx = threadIdx.x + it * CHUNK_NW * WAVE;
                    const int t = min(tile * CHUNK_T + idx / DCH, maxlen - 1);
                    pgid[it] = seqp[t >> rows.shift];
                }
            }
        }
    };
    auto tile_load = [&](int tile) {
        #pragma unroll
        for (int it = 0; it < NLD; it++) {
            const int idx = threadIdx.x + it * CHUNK_NW * WAVE;
            const int t = min(tile * CHUNK_T + idx / DCH, maxlen - 1);
            int64_t r = t;
            if constexpr (ROWS::kPaged)
                r = ((int64_t)pgid[it] << rows.shift)
                  + (t & ((1 << rows.shift) - 1));
            const int64_t off = r * kv_dim0 + (idx % DCH) * 8;
            kreg[it] = *reinterpret_cast<const Staged *>(kc + off);
            vreg[it] = *reinterpret_cast<const Staged *>(vc + off);
            if constexpr (Q8) {
                const int64_t so = r * nblk + (idx % DCH) * 8 / QB;
                kscl[it] = ks[so];
                vscl[it] = vs[so];
            }
        }
    };
    auto tile_store = [&](int buf) {
        #pragma unroll
        for (int it = 0; it < NLD; it++) {
            const int idx = threadIdx.x + it * CHUNK_NW * WAVE;
            const int t = idx / DCH, d = (idx % DCH) * 8;
            v8h_t kh, vh;
            if constexpr (Q8) {
                kh = q80_codes_f16(kreg[it], kscl[it]);
                vh = q80_codes_f16(vreg[it], vscl[it]);
            } else {
                kh = kreg[it];
                vh = vreg[it];
            }
            *reinterpret_cast<v8h_t *>(&sk[buf][t * KLD + d]) = kh;
            #pragma unroll
            for (int i = 0; i < 8; i++) sv[buf][(d + i) * VLD + t] = vh[i];
        }
    };

    for (int hg = 0; hg < kv_mul; hg += CHUNK_NW) {
        const bool active = hg + wave < kv_mul;  // wave-uniform
        const int h0 = kvh * kv_mul + hg + wave;

        // q * scale in f32, rounded to f16 once: the B operand for the pass
        v8h_t qf[hd / 16];
        #pragma unroll
        for (int kb = 0; kb < hd / 16; kb++) {
            float4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = x0;
            if (active && real) {
                const float *qp = q + (int64_t)b * q_ld + h0 * hd + kb * 16 + hi * 8;
                x0 = *reinterpret_cast<const float4 *>(qp);
                x1 = *reinterpret_cast<const float4 *>(qp + 4);
            }
            qf[kb] = v8h_t{
                (_Float16)mul_f32(x0.x, scale), (_Float16)mul_f32(x0.y, scale),
                (_Float16)mul_f32(x0.z, scale), (_Float16)mul_f32(x0.w, scale),
                (_Float16)mul_f32(x1.x, scale), (_Float16)mul_f32(x1.y, scale),
                (_Float16)mul_f32(x1.z, scale), (_Float16)mul_f32(x1.w, scale)};
        }

        v16f_t o[hd / 32];
        #pragma unroll
        for (int mb = 0; mb < hd / 32; mb++)
            #pragma unroll
            for (int r = 0; r < 16; r++) o[mb][r] = 0.0f;
        // this lane's half of the row's l (its 16 timesteps per tile); m is
        // the row's, equal in lane and lane^32
        float m = -1e30f, l = 0.0f;

        // double-buffered: tile i+S is in flight from the cache while tile i
        // is multiplied; one barrier per tile (the buffer stored to at the
        // end of an iteration was last read before the previous barrier)
        int tile = sp, buf = 0;
        page_fetch(tile);
        if (tile * CHUNK_T < maxlen) {
            tile_load(tile);
            page_fetch(tile + S);
            tile_store(0);
        }
        __syncthreads();
        for (; tile * CHUNK_T < maxlen; tile += S, buf ^= 1) {
            const bool more = (tile + S) * CHUNK_T < maxlen;
            if (more) {
                tile_load(tile + S);
                page_fetch(tile + 2 * S);
            }
            if (active) {
                const int t0 = tile * CHUNK_T;
                v16f_t s;
                #pragma unroll
                for (int r = 0; r < 16; r++) s[r] = 0.0f;
                #pragma unroll
                for (int kb = 0; kb < hd / 16; kb++) {
                    const v8h_t kf = *reinterpret_cast<const v8h_t *>(
                        &sk[buf][row * KLD + kb * 16 + hi * 8]);
                    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[kb], s,
                                                               0, 0, 0);
                }
                // only a tile that reaches past the run's shortest row masks
                const bool straddle = t0 + CHUNK_T > minlen;
                float mx = -1e30f;
                #pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (straddle && t >= plen) s[r] = -1e30f;
                    mx = fmaxf(mx, s[r]);
                }
                mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
                const float mn = fmaxf(m, mx);
                // exp(x - mn) as exp2(x * log2(e) - mn * log2(e)), one fma
                constexpr float LOG2E = 1.4426950408889634f;
                const float nmn = -mn * LOG2E;
                // m = -1e30 (nothing valid yet): l and o are 0, any finite
                // f does; the fma's rounding of 1e30-sized terms would not be
                const float f = m > -1e30f
                    ? __builtin_amdgcn_exp2f(fma_f32(m, LOG2E, nmn)) : 0.0f;
                float p[16], ls = 0.0f;
                #pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    // a masked weight is 0 by name: a row with nothing valid
                    // yet has mn = -1e30, where exp(s - mn) would be 1
                    p[r] = (straddle && t >= plen) ? 0.0f
                        : __builtin_amdgcn_exp2f(fma_f32(s[r], LOG2E, nmn));
                    ls += p[r];
                }
                l = l * f + ls;
                m = mn;
                v8h_t pf[2];
                #pragma unroll
                for (int c = 0; c < 2; c++)
                    #pragma unroll
                    for (int j = 0; j < 8; j++) pf[c][j] = (_Float16)p[8 * c + j];
                #pragma unroll
                for (int mb = 0; mb < hd / 32; mb++) {
                    #pragma unroll
                    for (int r = 0; r < 16; r++) o[mb][r] = mul_f32(o[mb][r], f);
                    #pragma unroll
                    for (int c = 0; c < 2; c++) {
                        const _Float16 *vp =
                            &sv[buf][(mb * 32 + row) * VLD + 16 * c + 4 * hi];
                        const v4h_t v0 = *reinterpret_cast<const v4h_t *>(vp);
                        const v4h_t v1 = *reinterpret_cast<const v4h_t *>(vp + 8);
                        const v8h_t vf = __builtin_shufflevector(
                            v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                        o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                            vf, pf[c], o[mb], 0, 0, 0);
                    }
                }
            }
            if (more) tile_store(buf ^ 1);
            __syncthreads();
        }

        if (active) {
            l += __shfl_xor(l, 32, WAVE);
            if (real) {
                // a row with no timestep in this split leaves m = -1e30,
                // l = 0, o = 0, as k_attn_split does
                const int64_t slot = ((int64_t)b * n_heads0 + h0) * S + sp;
                if (hi == 0) {
                    ml_scratch[slot * 2] = m;
                    ml_scratch[slot * 2 + 1] = l;
                }
                #pragma unroll
                for (int mb = 0; mb < hd / 32; mb++)
                    #pragma unroll
                    for (int g = 0; g < 4; g++)
                        *reinterpret_cast<float4 *>(
                            o_scratch + slot * hd + mb * 32 + 8 * g + 4 * hi) =
                            float4{o[mb][4 * g], o[mb][4 * g + 1],
                                   o[mb][4 * g + 2], o[mb][4 * g + 3]};
            }
        }
    }
}

// ------------------------------------------------- GQA-packed MFMA decode
// The decode-row producer of the split scratch: a decode row is a run of one,
// so what a workgroup can share is the kv_mul query heads of a KV head. They
// are the N dimension of the MFMA, and K/V is read once per (KV head, row)
// instead of once per query head. Grid (n_kv_heads0, B, S), 4 waves; nothing
// in it depends on positions. Split sp walks the 32-timestep tiles sp, sp+S,
// .. up to the tile that holds the row's position, and wave w takes every
// fourth of them: the waves split time (k_attn_chunk's split heads), each
// carries (m, l, O) of all heads, and they merge through LDS in wave order at
// the end. No barrier inside the timestep loop.
//
// Layouts (v_mfma_f32_16x16x32_f16): A[m][k] and B[k][n] hold k = 8*(lane>>4)
// + j in half j of lane (m or n) + 16*(lane>>4); C[m][n] holds n = lane&15,
// m = 4*(lane>>4) + r in register r. Scores are computed transposed,
// S^T = K Q^T (m = timestep, n = query head): the A fragment of a K row is 8
// consecutive halves of the cache row, one 16-byte load and no LDS, and a
// lane holds 4 scores of ONE head per 16-timestep half of the tile. The
// online softmax of a head is lane-local but for the exchanges with lane^16
// and lane^32. The lane's 8 weights of a tile, rounded to f16, are directly
// the B operand of O^T += V^T P^T over the timesteps
//   t(g, j) = 16*(j>>2) + 4*g + (j&3),  g = lane>>4, j = 0..7,
// because the MFMA only sums over k: the A operand V^T gathers the same
// timesteps. P never moves between lanes; O^T again holds the lane's head.
//
// V is d-contiguous in the cache and the A operand wants 8 timesteps of one
// d per lane. It goes through a wave-private LDS tile: lane (g, dc) loads the
// 8-element chunk dc of the rows t(g, 0..7) (whole 128- or 256-byte row
// pieces per 16 lanes), transposes its 8x8 halves in registers and stores
// one vector per d, so that row d of the tile holds the 32 timesteps in k
// order and a fragment is one 16-byte LDS read. A wave reads only what it
// wrote, in program order: no barrier. (head_dim 64 has 8 chunks per row:
// a lane takes half of the k group, 4 timesteps, and stores 8 bytes per d.)
//
// Prefetch: K and V of a wave's next tile are loaded into the other of two
// register sets before the current tile is multiplied (the loop is unrolled
// by the two sets), page ids one tile further ahead. Loads are never guarded:
// a timestep past the row's position re-reads the row of the position itself,
// in the last tile (masked: its weight is 0 by name) and in the one prefetch
// past it (never used), so no address past the position is formed and no
// unmapped page is looked up.
//
// Rounding points are k_attn_chunk's: q*scale (f32) -> f16 once, P -> f16
// per tile; scores, m, l and O accumulate in f32.
//
// Q80 form (KVT = int8_t, ROWS = Q80Rows<..>): the same kernel but for how a
// tile becomes MFMA operands, K and V entering as f16(code * scale)
// (q80_dword_f16). K: lane g of the four that hold a K row takes one
// contiguous quarter of it, hd/4 codes = one block or half of one, so one
// scale; fragment kb is its codes 8 kb .. 8 kb + 7, converted in registers
// before the MFMA, and q is permuted the same way. V: a row of the head is 8
// pieces of hd/8 codes; lane (vg, u, dc) = (lane & 3, (lane >> 2) & 1,
// lane >> 3) loads piece dc of the 4 consecutive rows 16 u + 4 vg + 0..3 and
// their scales (a load instruction reads 8 whole rows of the head; the 4
// rows lie in one page), converts, transposes in registers and stores 4
// halves per d into the same V^T tile. A tile set is 38 registers against 64
// at head_dim 128: the ring stays two sets and a third wave fits the SIMD.
typedef float v4f_t __attribute__((ext_vector_type(4)));

constexpr int GQA_T = 32;      // timesteps per tile = MFMA K of O^T += V^T P^T
constexpr int GQA_HEADS = 16;  // query heads per KV head served = MFMA N
constexpr int GQA_NW = 4;      // waves per workgroup
constexpr int GQA_VLD = GQA_T + 8;  // halves per V^T row: 16-byte rows, skewed

template <int VEC, typename KVT, typename ROWS>
__global__ void __launch_bounds__(GQA_NW * WAVE, 2)
k_attn_gqa(const float *__restrict__ q, int q_ld,
           const KVT *__restrict__ kc_all, const KVT *__restrict__ vc_all,
           const ROWS rows, int n_heads0, int kv_mul, int kv_dim0, float scale,
           float *__restrict__ ml_scratch, float *__restrict__ o_scratch) {
    constexpr bool Q8 = kKVQ80<KVT>;
    static_assert(Q8 || std::is_same_v<KVT, __half>,
                  "k_attn_gqa serves f16 and Q80 caches");
    constexpr int hd = VEC * WAVE;
    constexpr int KB = hd / 32;       // score MFMAs per 16 timesteps
    constexpr int DB = hd / 16;       // 16-row blocks of O^T
    constexpr int DCH = hd / 8;       // 16-byte chunks per cache row of the head
    constexpr int VP = Q8 ? 8 : DCH;  // pieces a V row of the head is staged in
    constexpr int NJ = VP / 2;        // timesteps a lane stages of V: 8 or 4
    constexpr int NG = NJ / 4;        // groups of 4 consecutive timesteps in them
    // Q80: dwords of codes a lane holds of a K row (a quarter of the head)
    // and of a V row (one of VP pieces)
    constexpr int KW = hd / 16, VW = hd / 32;
    typedef int KCodes __attribute__((ext_vector_type(4)));
    typedef int VCodes __attribute__((ext_vector_type(VW)));
    using VCol = _Float16 __attribute__((ext_vector_type(NJ)));
    // the V^T tiles of the waves; after the loop, the waves' O partials
    __shared__ __attribute__((aligned(16))) char smem[GQA_NW * hd * GQA_VLD * 2];
    __shared__ float sm[GQA_NW][GQA_HEADS], sl[GQA_NW][GQA_HEADS];
    static_assert(sizeof(smem) >= GQA_NW * GQA_HEADS * hd * sizeof(float),
                  "the O partials fit the V tiles");

    const int kvh = blockIdx.x;
    const int b = blockIdx.y;
    const int sp = blockIdx.z;
    const int S = gridDim.z;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int lane = threadIdx.x % WAVE;
    const int n = lane & 15;  // query head of the KV head; K row of a fragment
    const int g = lane >> 4;  // k group
    // V staging: k group, chunk of the row, and which NJ of the group's 8
    // (Q80: both halves of a k group sit in one half-wave, so that a store
    // instruction spreads over twice the LDS banks)
    const int vg = lane & 3;
    const int vdc = Q8 ? lane >> 3 : (lane >> 2) % DCH;
    const int vj0 = Q8 ? lane & 4 : (lane >> 2) / DCH * NJ;

    const int pos = rows.position(b);
    const int last = pos >> 5;  // the tile that holds the position
    using KVE = std::conditional_t<Q8, int8_t, _Float16>;
    const KVE *kc = reinterpret_cast<const KVE *>(kc_all)
                  + rows.cache_base(b) * kv_dim0 + kvh * hd;
    const KVE *vc = reinterpret_cast<const KVE *>(vc_all)
                  + rows.cache_base(b) * kv_dim0 + kvh * hd;
    // Q80: the scale planes, f16 [rows, kv_dim0/32], from the same cache row
    [[maybe_unused]] const int nblk = kv_dim0 / QB;
    [[maybe_unused]] const _Float16 *ks = nullptr, *vs = nullptr;
    if constexpr (Q8) {
        const int64_t sb = rows.cache_base(b) * nblk + kvh * (hd / QB);
        ks = reinterpret_cast<const _Float16 *>(rows.ks) + sb;
        vs = reinterpret_cast<const _Float16 *>(rows.vs) + sb;
    }
    _Float16 *sv = reinterpret_cast<_Float16 *>(smem) + wave * hd * GQA_VLD;

    // Paged: a K fragment row has its own page; a V group of 4 consecutive
    // timesteps starts at a multiple of 4 and lies in one page (P >= 4).
    // With pages of 32 rows or more the tile lies in one page: one uniform
    // id. A timestep past pos looks up the page of pos.
    struct Ids { int k[2], v[NG]; };
    struct TileH { v8h_t k[2][KB], v[NJ]; };
    // Q80: a quarter of each K row and a piece of 4 V rows as codes, and one
    // scale per row
    struct TileQ {
        KCodes k[2][KW / 4];
        VCodes v[NJ];
        _Float16 ks[2], vs[NJ];
    };
    using Tile = std::conditional_t<Q8, TileQ, TileH>;
    [[maybe_unused]] const int *seqp = nullptr;
    [[maybe_unused]] int pshift = 0;
    if constexpr (ROWS::kPaged) {
        seqp = rows.seq_pages(b);
        pshift = rows.shift;
    }
    // tile-local timestep of k index j of this lane's V group
    auto vt = [&](int j) { return 16 * (j >> 2) + 4 * vg + (j & 3); };
    auto fetch_ids = [&](int tile) {
        Ids id{};
        if constexpr (ROWS::kPaged) {
            const int t0 = tile * GQA_T;
            if (pshift >= 5) {
                const int x = seqp[min(t0, pos) >> pshift];
                id.k[0] = id.k[1] = x;
                #pragma unroll
                for (int c = 0; c < NG; c++) id.v[c] = x;
            } else {
                #pragma unroll
                for (int u = 0; u < 2; u++)
                    id.k[u] = seqp[min(t0 + 16 * u + n, pos) >> pshift];
                #pragma unroll
                for (int c = 0; c < NG; c++)
                    id.v[c] = seqp[min(t0 + vt(vj0 + 4 * c), pos) >> pshift];
            }
        }
        return id;
    };
    // cache row (relative to kc / vc) of timestep t <= pos
    auto row_of = [&](int t, int id) {
        if constexpr (ROWS::kPaged)
            return ((int64_t)id << pshift) + (t & ((1 << pshift) - 1));
        else
            return (int64_t)t;
    };
    auto load = [&](int tile, const Ids &id, Tile &x) {
        const int t0 = tile * GQA_T;
        if constexpr (Q8) {
            // K: the quarter g of the row (block g, or half of block g >> 1)
            // and its one scale; V: piece vdc of 4 consecutive rows, a scale
            // each. Both scales are read from the row the codes come from.
            #pragma unroll
            for (int u = 0; u < 2; u++) {
                const int t = min(t0 + 16 * u + n, pos);
                const int64_t r = row_of(t, id.k[u]);
                const int8_t *p = kc + r * kv_dim0 + 4 * KW * g;
                #pragma unroll
                for (int w = 0; w < KW / 4; w++)
                    x.k[u][w] = *reinterpret_cast<const KCodes *>(p + 16 * w);
                x.ks[u] = ks[r * nblk + 4 * KW * g / QB];
            }
            #pragma unroll
            for (int jj = 0; jj < NJ; jj++) {
                const int t = min(t0 + vt(vj0 + jj), pos);
                const int64_t r = row_of(t, id.v[0]);
                x.v[jj] = *reinterpret_cast<const VCodes *>(
                    vc + r * kv_dim0 + 4 * VW * vdc);
                x.vs[jj] = vs[r * nblk + 4 * VW * vdc / QB];
            }
        } else {
            #pragma unroll
            for (int u = 0; u < 2; u++) {
                const int t = min(t0 + 16 * u + n, pos);
                const _Float16 *p =
                    kc + row_of(t, id.k[u]) * kv_dim0 + 8 * g;
                #pragma unroll
                for (int kb = 0; kb < KB; kb++)
                    x.k[u][kb] = *reinterpret_cast<const v8h_t *>(p + 32 * kb);
            }
            #pragma unroll
            for (int jj = 0; jj < NJ; jj++) {
                const int t = min(t0 + vt(vj0 + jj), pos);
                x.v[jj] = *reinterpret_cast<const v8h_t *>(
                    vc + row_of(t, id.v[jj >> 2]) * kv_dim0 + 8 * vdc);
            }
        }
    };

    // q * scale in f32, rounded to f16 once: the B operand of the scores.
    // Heads at or past kv_mul are padding, never stored: they load the last
    // head (no guarded load, no wait per load) and scale it by 0.
    // The MFMA only sums over k, so which d a lane's half j of fragment kb is
    // is free as long as K and q agree: d = 32 kb + 8 g + j for an f16
    // cache, d = (hd/4) g + 8 kb + j for a Q80 one, where lane g holds one
    // contiguous quarter of the K row (one block, or half of one).
    constexpr int QG = Q8 ? hd / 4 : 8, QKB = Q8 ? 8 : 32;
    const float qs = n < kv_mul ? scale : 0.0f;
    const float *qp = q + (int64_t)b * q_ld
                    + (kvh * kv_mul + min(n, kv_mul - 1)) * hd + QG * g;
    v8h_t qf[KB];
    #pragma unroll
    for (int kb = 0; kb < KB; kb++) {
        const float4 x0 = *reinterpret_cast<const float4 *>(qp + QKB * kb);
        const float4 x1 = *reinterpret_cast<const float4 *>(qp + QKB * kb + 4);
        qf[kb] = v8h_t{
            (_Float16)mul_f32(x0.x, qs), (_Float16)mul_f32(x0.y, qs),
            (_Float16)mul_f32(x0.z, qs), (_Float16)mul_f32(x0.w, qs),
            (_Float16)mul_f32(x1.x, qs), (_Float16)mul_f32(x1.y, qs),
            (_Float16)mul_f32(x1.z, qs), (_Float16)mul_f32(x1.w, qs)};
    }

    v4f_t o[DB];
    #pragma unroll
    for (int db = 0; db < DB; db++) o[db] = v4f_t{0.f, 0.f, 0.f, 0.f};
    // m is the head's, equal in the four lanes that hold it; l is this
    // lane's quarter (its 8 timesteps per tile), summed at the end
    float m = -1e30f, l = 0.0f;

    auto compute = [&](int tile, const Tile &x) {
        // V^T into the wave's tile: row d = the 32 timesteps in k order
        if constexpr (Q8) {
            // the lane's piece of 4 consecutive rows, each times its scale,
            // transposed in registers: 4 halves (8 bytes) per d
            #pragma unroll
            for (int w = 0; w < VW; w++) {
                v4h_t h[NJ];
                #pragma unroll
                for (int jj = 0; jj < NJ; jj++)
                    h[jj] = q80_dword_f16(x.v[jj][w], x.vs[jj]);
                #pragma unroll
                for (int c = 0; c < 4; c++) {
                    VCol col;
                    #pragma unroll
                    for (int jj = 0; jj < NJ; jj++) col[jj] = h[jj][c];
                    *reinterpret_cast<VCol *>(
                        &sv[(4 * VW * vdc + 4 * w + c) * GQA_VLD + 8 * vg
                            + vj0]) = col;
                }
            }
        } else {
            #pragma unroll
            for (int i = 0; i < 8; i++) {
                VCol col;
                #pragma unroll
                for (int jj = 0; jj < NJ; jj++) col[jj] = x.v[jj][i];
                *reinterpret_cast<VCol *>(
                    &sv[(8 * vdc + i) * GQA_VLD + 8 * vg + vj0]) = col;
            }
        }
        // the fragment reads below are other lanes' stores: keep the order
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        v4f_t s[2];
        #pragma unroll
        for (int u = 0; u < 2; u++) {
            s[u] = v4f_t{0.f, 0.f, 0.f, 0.f};
            #pragma unroll
            for (int kb = 0; kb < KB; kb++) {
                v8h_t kf;
                if constexpr (Q8) {
                    // codes 8 kb .. 8 kb + 7 of the lane's quarter
                    const int w = 2 * kb;
                    const v4h_t lo = q80_dword_f16(x.k[u][w / 4][w % 4],
                                                   x.ks[u]);
                    const v4h_t hi = q80_dword_f16(x.k[u][w / 4][w % 4 + 1],
                                                   x.ks[u]);
                    kf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                } else {
                    kf = x.k[u][kb];
                }
                s[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                    kf, qf[kb], s[u], 0, 0, 0);
            }
        }
        // only the tile that holds the position masks
        const bool edge = tile == last;
        const int tl = tile * GQA_T + 4 * g;  // timestep of s[0][0]
        float mx = -1e30f;
        #pragma unroll
        for (int u = 0; u < 2; u++)
            #pragma unroll
            for (int r = 0; r < 4; r++) {
                if (edge && tl + 16 * u + r > pos) s[u][r] = -1e30f;
                mx = fmaxf(mx, s[u][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
        mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
        // the tile's first timestep is at or below pos: mx is a real score
        const float mn = fmaxf(m, mx);
        constexpr float LOG2E = 1.4426950408889634f;
        const float nmn = -mn * LOG2E;
        // m = -1e30 (the wave's first tile): l and o are 0, any finite f does
        const float f = m > -1e30f
            ? __builtin_amdgcn_exp2f(fma_f32(m, LOG2E, nmn)) : 0.0f;
        v8h_t pf;
        float ls = 0.0f;
        #pragma unroll
        for (int u = 0; u < 2; u++)
            #pragma unroll
            for (int r = 0; r < 4; r++) {
                // a masked weight is 0 by name, not left to exp: its bits
                // are cleared (a select would put a branch around each exp)
                const unsigned keep =
                    (edge && tl + 16 * u + r > pos) ? 0u : ~0u;
                const float p = __uint_as_float(keep & __float_as_uint(
                    __builtin_amdgcn_exp2f(fma_f32(s[u][r], LOG2E, nmn))));
                ls += p;
                pf[4 * u + r] = (_Float16)p;
            }
        l = fma_f32(l, f, ls);
        m = mn;
        #pragma unroll
        for (int db = 0; db < DB; db++) {
            #pragma unroll
            for (int r = 0; r < 4; r++) o[db][r] = mul_f32(o[db][r], f);
            const v8h_t vf = *reinterpret_cast<const v8h_t *>(
                &sv[(16 * db + n) * GQA_VLD + 8 * g]);
            o[db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[db],
                                                           0, 0, 0);
        }
        // the next tile's stores come behind these reads
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    };

    // a wave with no tile keeps m = -1e30, l = 0, o = 0
    const int step = GQA_NW * S;
    int tile = sp + S * wave;
    if (tile <= last) {
        Tile ta, tb;
        Ids id = fetch_ids(tile);
        load(tile, id, ta);
        id = fetch_ids(tile + step);
        for (;;) {
            // ids first: waiting for them later must not drain the K/V loads
            Ids nid = fetch_ids(tile + 2 * step);
            load(tile + step, id, tb);
            id = nid;
            compute(tile, ta);
            tile += step;
            if (tile > last) break;
            nid = fetch_ids(tile + 2 * step);
            load(tile + step, id, ta);
            id = nid;
            compute(tile, tb);
            tile += step;
            if (tile > last) break;
        }
    }

    // merge the four waves in wave order, as k_attn_split does
    l += __shfl_xor(l, 16, WAVE);
    l += __shfl_xor(l, 32, WAVE);
    __syncthreads();  // every wave is done with its V tile
    float *so = reinterpret_cast<float *>(smem);  // [wave][head][hd]
    if (n < kv_mul) {
        if (g == 0) { sm[wave][n] = m; sl[wave][n] = l; }
        #pragma unroll
        for (int db = 0; db < DB; db++)
            *reinterpret_cast<v4f_t *>(
                &so[(wave * GQA_HEADS + n) * hd + 16 * db + 4 * g]) = o[db];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kv_mul * hd; e += GQA_NW * WAVE) {
        const int hn = e / hd, d = e % hd;
        float M = -1e30f;
        #pragma unroll
        for (int w = 0; w < GQA_NW; w++) M = fmaxf(M, sm[w][hn]);
        // all four empty: M = -1e30, every weight 1, l = 0 and o = 0
        float L = 0.0f, acc = 0.0f;
        #pragma unroll
        for (int w = 0; w < GQA_NW; w++) {
            const float fw = __expf(sm[w][hn] - M);
            L = fmaf(sl[w][hn], fw, L);
            acc = fmaf(so[(w * GQA_HEADS + hn) * hd + d], fw, acc);
        }
        const int64_t slot =
            ((int64_t)b * n_heads0 + kvh * kv_mul + hn) * S + sp;
        o_scratch[slot * hd + d] = acc;
        if (d == 0) {
            ml_scratch[slot * 2] = M;
            ml_scratch[slot * 2 + 1] = L;
        }
    }
}

// ------------------------------------------------- shared-prefix attention
// The producer of the split scratch for what several sequences have in
// common: decode rows whose sequences start with the same run of pool pages
// (a system prompt mapped into many slots) attend that run once per group
// instead of once per row. The host groups the rows (models/rows.py
// prefix_groups) and stages three tables: pre_rows int32 [B, 2] = {group or
// -1, plen} per batch row, groups int32 [G, 2] = {first, count} into members
// int32 [..] (batch-row indices), and the live group count on the device.
//
// Grid (n_kv_heads0, G, S_pre), 4 waves; nothing in it depends on the
// grouping or on positions, a workgroup at or past the live group count
// leaves on a uniform branch, so a captured step replays for any grouping.
// Column c of a workgroup is (member c / kv_mul, query head c % kv_mul of the
// KV head): up to 128 columns, wave w owns columns 32w .. 32w+31 as the N
// dimension of v_mfma_f32_32x32x16_f16. Split sp walks the 32-timestep tiles
// sp, sp + S_pre, .. below plen. Every K/V tile is staged in LDS once per
// workgroup (k_attn_chunk's tiles: K [t][d], V transposed [d][t], two
// buffers, one barrier per tile) and read by all four waves: a K/V byte
// leaves the cache once per 128 columns, which is why this kernel stages
// through LDS and not through registers as k_attn_gqa does. Page ids come
// from the first member's list, one tile ahead of the loads.
//
// No causal mask: every column sees the whole prefix. Only the tile that
// holds plen masks, uniformly (t >= plen; possible with pages below 32 rows
// only), its weights 0 by name. Math, layouts and rounding points are
// k_attn_chunk's (S^T = K Q^T, lane-local online softmax, registers 8c..8c+7
// of the scores as the B operand of O^T += V^T P^T).
//
// The tables are the host's, but no table can send a load or store astray:
// the group is clamped to the member list, members to the batch, plen to the
// smallest member position (a shared page is full and read-only, so a valid
// plen lies at or below it), and K/V are only ever found through the first
// member's page list below that plen.
//
// The rest of a row's history is the suffix: k_attn_gqa over SuffixRows,
// which moves the row's time origin to plen (K was roped before it was
// cached, so nothing else changes), filling the ordinary split scratch.
// k_attn_combine_pre merges both sets of partials: the split of a softmax at
// plen is the same exact (m, l, o) algebra as the split across S.
struct SuffixRows : PagedRows {
    const int *pre;  // pre_rows: int32 [B, 2] = {group or -1, plen}
    __device__ int plen(int b) const {
        return min(max(pre[2 * b + 1], 0), rows[2 * b + 1]);
    }
    __device__ int position(int b) const { return rows[2 * b + 1] - plen(b); }
    __device__ const int *seq_pages(int b) const {
        return pages + rows[2 * b] + (plen(b) >> shift);
    }
    __device__ int64_t cache_row(int b, int t) const {
        return ((int64_t)seq_pages(b)[t >> shift] << shift)
             + (t & ((1 << shift) - 1));
    }
};

constexpr int PRE_T = 32;      // timesteps per tile = MFMA M of the scores
constexpr int PRE_NW = 4;      // waves per workgroup
constexpr int PRE_COLS = 128;  // (member, head) columns per workgroup
constexpr int PRE_HEADS = 16;  // kv_mul served

template <int VEC, typename KVT, typename ROWS>
__global__ void __launch_bounds__(PRE_NW * WAVE, 2)
k_attn_prefix(const float *__restrict__ q, int q_ld,
              const KVT *__restrict__ kc_all, const KVT *__restrict__ vc_all,
              const ROWS rows, const int *__restrict__ pre_rows,
              const int *__restrict__ groups, const int *__restrict__ members,
              int n_members, const int *__restrict__ n_groups, int batch,
              int n_heads0, int kv_mul, int kv_dim0, float scale,
              float *__restrict__ ml_scratch, float *__restrict__ o_scratch) {
    constexpr bool Q8 = kKVQ80<KVT>;
    static_assert(ROWS::kPaged, "a shared prefix is a run of pool pages");
    constexpr int hd = VEC * WAVE;
    constexpr int KLD = hd + 8;     // halves per K row: 16-byte rows, 4-bank skew
    constexpr int VLD = PRE_T + 4;  // halves per V^T row (one d): 8-byte rows
    constexpr int DCH = hd / 8;     // 16-byte chunks per cache row of the head
    constexpr int NLD = PRE_T * DCH / (PRE_NW * WAVE);  // chunks per thread
    static_assert(NLD * PRE_NW * WAVE == PRE_T * DCH, "tile / threads");
    __shared__ __attribute__((aligned(16))) _Float16 sk[2][PRE_T * KLD];
    __shared__ __attribute__((aligned(16))) _Float16 sv[2][hd * VLD];
    __shared__ int smin[PRE_NW];

    const int grp = blockIdx.y;
    if (grp >= n_groups[0]) return;  // uniform: no such group in this step
    const int kvh = blockIdx.x;
    const int sp = blockIdx.z;
    const int S = gridDim.z;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int lane = threadIdx.x % WAVE;
    const int row = lane & 31;  // column of the wave (B / C operand column)
    const int hi = lane >> 5;

    // the group, clamped to the member list and to the columns there are
    const int first = min(max(groups[2 * grp], 0), n_members - 1);
    const int count = min(min(groups[2 * grp + 1], n_members - first),
                          PRE_COLS / kv_mul);
    if (count < 1) return;  // uniform
    const int ncols = count * kv_mul;
    auto member = [&](int i) {
        return min(max(members[first + i], 0), batch - 1);
    };
    const int b0 = __builtin_amdgcn_readfirstlane(member(0));

    // plen: the first member's, at most the smallest position of the group
    int mp = (int)threadIdx.x < count ? rows.position(member(threadIdx.x))
                                      : 0x7fffffff;
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        mp = min(mp, __shfl_xor(mp, off, WAVE));
    if (lane == 0) smin[wave] = mp;
    __syncthreads();
    const int plen = __builtin_amdgcn_readfirstlane(
        min(max(pre_rows[2 * b0 + 1], 0),
            min(min(smin[0], smin[1]), min(smin[2], smin[3]))));

    // this lane's column
    const int col = 32 * wave + row;
    const bool real = col < ncols;        // else padding: q = 0, never written
    const bool active = 32 * wave < ncols;  // wave-uniform
    const int b = member(real ? col / kv_mul : 0);
    const int h0 = kvh * kv_mul + (real ? col % kv_mul : 0);

    const KVT *kc = kc_all + kvh * hd;
    const KVT *vc = vc_all + kvh * hd;
    // Q80: the scale planes, f16 [rows, kv_dim0/32], from the same cache row
    [[maybe_unused]] const int nblk = kv_dim0 / QB;
    [[maybe_unused]] const _Float16 *ks = nullptr, *vs = nullptr;
    if constexpr (Q8) {
        ks = reinterpret_cast<const _Float16 *>(rows.ks) + kvh * (hd / QB);
        vs = reinterpret_cast<const _Float16 *>(rows.vs) + kvh * (hd / QB);
    }

    // staging, as k_attn_chunk: a thread holds NLD 8-element chunks of the K
    // tile and of the V tile between their global load and their LDS store,
    // 16 bytes of f16 or 8 codes and their block's scale. A timestep at or
    // past plen (last tile only) re-reads row plen-1: valid, masked below.
    // With pages of 32 rows or more a tile lies in one page: one uniform id.
    using Staged = std::conditional_t<Q8, int2, v8h_t>;
    Staged kreg[NLD], vreg[NLD];
    [[maybe_unused]] _Float16 kscl[NLD], vscl[NLD];
    int pgid[NLD];  // page of each chunk of the next tile_load
    const int pshift = rows.shift;
    const int *seqp =
        rows.pages + __builtin_amdgcn_readfirstlane(rows.rows[2 * b0]);
    auto page_fetch = [&](int tile) {
        if (tile * PRE_T >= plen) return;  // no such tile
        if (pshift >= 5) {
            const int id = seqp[(tile * PRE_T) >> pshift];
            #pragma unroll
            for (int it = 0; it < NLD; it++) pgid[it] = id;
        } else {
            #pragma unroll
            for (int it = 0; it < NLD; it++) {
                const int idx = threadIdx.x + it * PRE_NW * WAVE;
                const int t = min(tile * PRE_T + idx / DCH, plen - 1);
                pgid[it] = seqp[t >> pshift];
            }
        }
    };
    auto tile_load = [&](int tile) {
        #pragma unroll
        for (int it = 0; it < NLD; it++) {
            const int idx = threadIdx.x + it * PRE_NW * WAVE;
            const int t = min(tile * PRE_T + idx / DCH, plen - 1);
            const int64_t r = ((int64_t)pgid[it] << pshift)
                            + (t & ((1 << pshift) - 1));
            const int64_t off = r * kv_dim0 + (idx % DCH) * 8;
            kreg[it] = *reinterpret_cast<const Staged *>(kc + off);
            vreg[it] = *reinterpret_cast<const Staged *>(vc + off);
            if constexpr (Q8) {
                const int64_t so = r * nblk + (idx % DCH) * 8 / QB;
                kscl[it] = ks[so];
                vscl[it] = vs[so];
            }
        }
    };
    auto tile_store = [&](int buf) {
        #pragma unroll
        for (int it = 0; it < NLD; it++) {
            const int idx = threadIdx.x + it * PRE_NW * WAVE;
            const int t = idx / DCH, d = (idx % DCH) * 8;
            v8h_t kh, vh;
            if constexpr (Q8) {
                kh = q80_codes_f16(kreg[it], kscl[it]);
                vh = q80_codes_f16(vreg[it], vscl[it]);
            } else {
                kh = kreg[it];
                vh = vreg[it];
            }
            *reinterpret_cast<v8h_t *>(&sk[buf][t * KLD + d]) = kh;
            #pragma unroll
            for (int i = 0; i < 8; i++) sv[buf][(d + i) * VLD + t] = vh[i];
        }
    };

    // q * scale in f32, rounded to f16 once: the B operand of the scores
    v8h_t qf[hd / 16];
    #pragma unroll
    for (int kb = 0; kb < hd / 16; kb++) {
        float4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = x0;
        if (real) {
            const float *qp = q + (int64_t)b * q_ld + h0 * hd + kb * 16 + hi * 8;
            x0 = *reinterpret_cast<const float4 *>(qp);
            x1 = *reinterpret_cast<const float4 *>(qp + 4);
        }
        qf[kb] = v8h_t{
            (_Float16)mul_f32(x0.x, scale), (_Float16)mul_f32(x0.y, scale),
            (_Float16)mul_f32(x0.z, scale), (_Float16)mul_f32(x0.w, scale),
            (_Float16)mul_f32(x1.x, scale), (_Float16)mul_f32(x1.y, scale),
            (_Float16)mul_f32(x1.z, scale), (_Float16)mul_f32(x1.w, scale)};
    }

    v16f_t o[hd / 32];
    #pragma unroll
    for (int mb = 0; mb < hd / 32; mb++)
        #pragma unroll
        for (int r = 0; r < 16; r++) o[mb][r] = 0.0f;
    // this lane's half of the column's l (its 16 timesteps per tile); m is
    // the column's, equal in lane and lane^32
    float m = -1e30f, l = 0.0f;

    // double-buffered: tile i+S is in flight from the cache while tile i is
    // multiplied; one barrier per tile (the buffer stored to at the end of an
    // iteration was last read before the previous barrier)
    int tile = sp, buf = 0;
    page_fetch(tile);
    if (tile * PRE_T < plen) {
        tile_load(tile);
        page_fetch(tile + S);
        tile_store(0);
    }
    __syncthreads();
    for (; tile * PRE_T < plen; tile += S, buf ^= 1) {
        const bool more = (tile + S) * PRE_T < plen;
        if (more) {
            tile_load(tile + S);
            page_fetch(tile + 2 * S);
        }
        if (active) {
            const int t0 = tile * PRE_T;
            v16f_t s;
            #pragma unroll
            for (int r = 0; r < 16; r++) s[r] = 0.0f;
            #pragma unroll
            for (int kb = 0; kb < hd / 16; kb++) {
                const v8h_t kf = *reinterpret_cast<const v8h_t *>(
                    &sk[buf][row * KLD + kb * 16 + hi * 8]);
                s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[kb], s,
                                                           0, 0, 0);
            }
            // only the tile that holds plen masks, for every column alike
            const bool edge = t0 + PRE_T > plen;
            float mx = -1e30f;
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (edge && t >= plen) s[r] = -1e30f;
                mx = fmaxf(mx, s[r]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
            // the tile's first timestep is below plen: mx is a real score
            const float mn = fmaxf(m, mx);
            constexpr float LOG2E = 1.4426950408889634f;
            const float nmn = -mn * LOG2E;
            // m = -1e30 (the first tile): l and o are 0, any finite f does
            const float f = m > -1e30f
                ? __builtin_amdgcn_exp2f(fma_f32(m, LOG2E, nmn)) : 0.0f;
            float p[16], ls = 0.0f;
            #pragma unroll
            for (int r = 0; r < 16; r++) {
                const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                // a masked weight is 0 by name, not left to exp
                p[r] = (edge && t >= plen) ? 0.0f
                    : __builtin_amdgcn_exp2f(fma_f32(s[r], LOG2E, nmn));
                ls += p[r];
            }
            l = fma_f32(l, f, ls);
            m = mn;
            v8h_t pf[2];
            #pragma unroll
            for (int c = 0; c < 2; c++)
                #pragma unroll
                for (int j = 0; j < 8; j++) pf[c][j] = (_Float16)p[8 * c + j];
            #pragma unroll
            for (int mb = 0; mb < hd / 32; mb++) {
                #pragma unroll
                for (int r = 0; r < 16; r++) o[mb][r] = mul_f32(o[mb][r], f);
                #pragma unroll
                for (int c = 0; c < 2; c++) {
                    const _Float16 *vp =
                        &sv[buf][(mb * 32 + row) * VLD + 16 * c + 4 * hi];
                    const v4h_t v0 = *reinterpret_cast<const v4h_t *>(vp);
                    const v4h_t v1 = *reinterpret_cast<const v4h_t *>(vp + 8);
                    const v8h_t vf = __builtin_shufflevector(
                        v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
                    o[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
                        vf, pf[c], o[mb], 0, 0, 0);
                }
            }
        }
        if (more) tile_store(buf ^ 1);
        __syncthreads();
    }

    if (active) {
        l += __shfl_xor(l, 32, WAVE);
        if (real) {
            // a split with no tile leaves m = -1e30, l = 0, o = 0
            const int64_t slot = ((int64_t)b * n_heads0 + h0) * S + sp;
            if (hi == 0) {
                ml_scratch[slot * 2] = m;
                ml_scratch[slot * 2 + 1] = l;
            }
            #pragma unroll
            for (int mb = 0; mb < hd / 32; mb++)
                #pragma unroll
                for (int g = 0; g < 4; g++)
                    *reinterpret_cast<float4 *>(
                        o_scratch + slot * hd + mb * 32 + 8 * g + 4 * hi) =
                        float4{o[mb][4 * g], o[mb][4 * g + 1],
                               o[mb][4 * g + 2], o[mb][4 * g + 3]};
        }
    }
}

// Stage 2 of the shared-prefix attention: k_attn_combine over the S suffix
// partials of (b, h) and then, for a row with a prefix (plen > 0), its S_pre
// prefix partials, in that fixed order. An ungrouped row's prefix scratch is
// never read, so nothing has to be neutral-filled for it.
template <int VEC, bool QUANT>
__global__ void k_attn_combine_pre(const float *__restrict__ ml_scratch,
                                   const float *__restrict__ o_scratch,
                                   const float *__restrict__ pre_ml,
                                   const float *__restrict__ pre_o,
                                   const int *__restrict__ pre_rows,
                                   float *__restrict__ y,
                                   int8_t *__restrict__ zq,
                                   float *__restrict__ zs,
                                   float *__restrict__ zbs,
                                   int n_heads0, int S, int S_pre) {
    const int h0 = blockIdx.x;
    const int b = blockIdx.y;
    const int hd = VEC * WAVE;  // blockDim.x == hd
    const int64_t base = ((int64_t)b * n_heads0 + h0) * S;
    const int64_t pbase = ((int64_t)b * n_heads0 + h0) * S_pre;
    const int P = pre_rows[2 * b + 1] > 0 ? S_pre : 0;  // block-uniform
    float M = -1e30f;
    for (int sp = 0; sp < S; sp++)
        M = fmaxf(M, ml_scratch[(base + sp) * 2]);
    for (int sp = 0; sp < P; sp++)
        M = fmaxf(M, pre_ml[(pbase + sp) * 2]);
    float L = 0.0f;
    for (int sp = 0; sp < S; sp++)
        L += ml_scratch[(base + sp) * 2 + 1] * __expf(ml_scratch[(base + sp) * 2] - M);
    for (int sp = 0; sp < P; sp++)
        L += pre_ml[(pbase + sp) * 2 + 1] * __expf(pre_ml[(pbase + sp) * 2] - M);
    const float invL = 1.0f / L;
    const int i = threadIdx.x;
    float acc = 0.0f;
    for (int sp = 0; sp < S; sp++)
        acc += o_scratch[(base + sp) * hd + i]
             * __expf(ml_scratch[(base + sp) * 2] - M);
    for (int sp = 0; sp < P; sp++)
        acc += pre_o[(pbase + sp) * hd + i]
             * __expf(pre_ml[(pbase + sp) * 2] - M);
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

// Stage 2 for every producer of the split scratch; zq selects the Q80 form.
template <int V>
static void combine_launch(torch::Tensor &ml_scratch, torch::Tensor &o_scratch,
                           float *yp, int8_t *zqp, float *zsp, float *zbsp,
                           int64_t batch, int64_t n_heads0, int64_t splits) {
    auto combine = [&](auto quant_const) {
        hipLaunchKernelGGL((k_attn_combine<V, decltype(quant_const)::value>),
                           dim3(n_heads0, batch), dim3(V * WAVE), 0,
                           cur_stream(), ml_scratch.data_ptr<float>(),
                           o_scratch.data_ptr<float>(), yp, zqp, zsp, zbsp,
                           (int)n_heads0, (int)splits);
    };
    if (zqp) combine(std::true_type{});
    else combine(std::false_type{});
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
        combine_launch<V>(ml_scratch, o_scratch, yp, zqp, zsp, zbsp, batch,
                          n_heads0, splits);
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

// Prompt-chunk attention: k_attn_chunk fills the split scratch, the combine
// finishes as for k_attn_split. `runs` is null for the single sequence (the
// batch is one run). What the host can see is checked here; the contents of
// the row and run tables are the caller's (models/rows.py row_runs), and the
// kernel clamps a run to the batch and to 32 rows.
template <typename ROWS>
static void attn_chunk_launch(const char *name, const char *other,
                              torch::Tensor &q, int64_t q_ld, torch::Tensor &kc,
                              torch::Tensor &vc, torch::Tensor &y, ROWS rows,
                              const int *runs, int64_t n_runs, int64_t batch,
                              int64_t n_heads0, int64_t kv_mul,
                              int64_t head_dim, int64_t splits,
                              torch::Tensor &ml_scratch,
                              torch::Tensor &o_scratch, OptTensor &zq,
                              OptTensor &zs, OptTensor &zbs,
                              const OptTensor &k_scales,
                              const OptTensor &v_scales) {
    CHECK_CUDA(q);
    const bool f16 = kc.scalar_type() == at::kHalf
                  && vc.scalar_type() == at::kHalf;
    const bool q80 = kc.scalar_type() == at::kChar
                  && vc.scalar_type() == at::kChar;
    TORCH_CHECK(f16 || q80, name, " serves a float16 or an int8 (Q80) KV "
                "cache: use ", other, " for a float32 cache");
    TORCH_CHECK(q80 || (!k_scales.has_value() && !v_scales.has_value()), name,
                " takes k_scales / v_scales with an int8 (Q80) KV cache only");
    TORCH_CHECK(f16 || (k_scales.has_value() && v_scales.has_value()), name,
                ": an int8 (Q80) KV cache needs k_scales= and v_scales=");
    const KVScales sc = kv_scales(kc, vc, k_scales, v_scales);
    TORCH_CHECK(head_dim == 64 || head_dim == 128, name,
                " serves head_dim 64 and 128 (got ", head_dim, "): use ", other);
    TORCH_CHECK(batch >= 1 && n_runs >= 1 && batch <= n_runs * CHUNK_ROWS, name,
                ": a run holds at most ", CHUNK_ROWS, " rows (", batch,
                " rows in ", n_runs, " runs): cut it, or use ", other);
    TORCH_CHECK(kv_mul >= 1 && n_heads0 % kv_mul == 0 && splits >= 1
                && q_ld % 4 == 0 && kc.dim() == 2 && kc.is_contiguous()
                && vc.is_contiguous() && kc.sizes() == vc.sizes()
                && kc.size(1) == n_heads0 / kv_mul * head_dim,
                name, ": contiguous caches [rows, n_kv_heads0 * head_dim], "
                "n_heads0 a multiple of kv_mul, q_ld a multiple of 4");
    const int64_t slots = batch * n_heads0 * splits;
    TORCH_CHECK(ml_scratch.numel() >= slots * 2
                && o_scratch.numel() >= slots * head_dim,
                name, ": split scratch too small for ", slots, " partials");
    const bool quant = zq.has_value();
    float *yp = quant ? nullptr : y.data_ptr<float>();
    int8_t *zqp = quant ? zq->data_ptr<int8_t>() : nullptr;
    float *zsp = quant ? zs->data_ptr<float>() : nullptr;
    float *zbsp = quant ? zbs->data_ptr<float>() : nullptr;
    const dim3 grid(n_heads0 / kv_mul, n_runs, splits);
    with_head_vec(head_dim, [&](auto vec_const) {
        constexpr int V = decltype(vec_const)::value;
        with_kv_ptrs(kc, vc, [&](auto *kcp, auto *vcp) {
            using KVT = std::remove_pointer_t<decltype(kcp)>;
            auto launch = [&](auto krows) {
                hipLaunchKernelGGL((k_attn_chunk<V, KVT, decltype(krows)>),
                                   grid, dim3(CHUNK_NW * WAVE), 0,
                                   cur_stream(), q.data_ptr<float>(),
                                   (int)q_ld, kcp, vcp, krows, runs,
                                   (int)batch, (int)n_heads0, (int)kv_mul,
                                   (int)kc.size(1),
                                   1.0f / sqrtf((float)head_dim),
                                   ml_scratch.data_ptr<float>(),
                                   o_scratch.data_ptr<float>());
            };
            if constexpr (kKVQ80<KVT>)
                launch(Q80Rows<ROWS>{rows, sc.k, sc.v});
            else if constexpr (std::is_same_v<KVT, __half>)
                launch(rows);
        });
        combine_launch<V>(ml_scratch, o_scratch, yp, zqp, zsp, zbsp, batch,
                          n_heads0, splits);
    });
}

// attn for a prompt chunk of one sequence: rows 0..batch-1 are one run.
void attn_chunk(torch::Tensor q, int64_t q_ld, torch::Tensor kc,
                torch::Tensor vc, torch::Tensor y, torch::Tensor pos,
                int64_t batch, int64_t n_heads0, int64_t kv_mul,
                int64_t head_dim, int64_t splits, torch::Tensor ml_scratch,
                torch::Tensor o_scratch, OptTensor zq = c10::nullopt,
                OptTensor zs = c10::nullopt, OptTensor zbs = c10::nullopt,
                OptTensor k_scales = c10::nullopt,
                OptTensor v_scales = c10::nullopt) {
    attn_chunk_launch("attn_chunk", "attn", q, q_ld, kc, vc, y,
                      SeqRows{pos.data_ptr<int>()}, nullptr, 1, batch, n_heads0,
                      kv_mul, head_dim, splits, ml_scratch, o_scratch, zq, zs,
                      zbs, k_scales, v_scales);
}

// attn_chunk for 1..128 rows of one sequence: ceil(batch / 32) runs in one
// launch, cut by the kernel (WideRows); each run's workgroups walk only the
// tiles below that run's longest row. The scratch holds batch * n_heads0 *
// splits partials. (attn_chunk itself keeps refusing more than one run.)
void attn_chunk_wide(torch::Tensor q, int64_t q_ld, torch::Tensor kc,
                     torch::Tensor vc, torch::Tensor y, torch::Tensor pos,
                     int64_t batch, int64_t n_heads0, int64_t kv_mul,
                     int64_t head_dim, int64_t splits, torch::Tensor ml_scratch,
                     torch::Tensor o_scratch, OptTensor zq = c10::nullopt,
                     OptTensor zs = c10::nullopt, OptTensor zbs = c10::nullopt,
                     OptTensor k_scales = c10::nullopt,
                     OptTensor v_scales = c10::nullopt) {
    TORCH_CHECK(batch >= 1 && batch <= 4 * CHUNK_ROWS,
                "attn_chunk_wide takes 1..128 rows of one sequence");
    TORCH_CHECK(q.numel() >= (batch - 1) * q_ld + n_heads0 * head_dim,
                "attn_chunk_wide: q shorter than `batch` rows");
    attn_chunk_launch("attn_chunk_wide", "attn", q, q_ld, kc, vc, y,
                      WideRows{pos.data_ptr<int>()}, nullptr,
                      ceil_div(batch, CHUNK_ROWS), batch, n_heads0, kv_mul,
                      head_dim, splits, ml_scratch, o_scratch, zq, zs, zbs,
                      k_scales, v_scales);
}

// A run table as the kernel reads it: int32 [>= n_runs, 2] = {first batch
// row, row count}, each run consecutive rows of one sequence.
static const int *run_table(const torch::Tensor &runs, int64_t n_runs,
                            const torch::Tensor &kc, const char *other) {
    TORCH_CHECK(runs.is_cuda() && runs.scalar_type() == at::kInt
                && runs.dim() == 2 && runs.size(1) == 2 && runs.is_contiguous()
                && n_runs >= 1 && runs.size(0) >= n_runs
                && runs.device() == kc.device(),
                "run table must be a contiguous int32 [>= n_runs, 2] on the "
                "cache's device (or use ", other, ")");
    return runs.data_ptr<int>();
}

// attn_rows with the rows grouped into runs.
void attn_chunk_rows(torch::Tensor q, int64_t q_ld, torch::Tensor kc,
                     torch::Tensor vc, torch::Tensor y, torch::Tensor rows,
                     torch::Tensor runs, int64_t n_runs, int64_t batch,
                     int64_t n_heads0, int64_t kv_mul, int64_t head_dim,
                     int64_t splits, torch::Tensor ml_scratch,
                     torch::Tensor o_scratch, OptTensor zq = c10::nullopt,
                     OptTensor zs = c10::nullopt, OptTensor zbs = c10::nullopt,
                     OptTensor k_scales = c10::nullopt,
                     OptTensor v_scales = c10::nullopt) {
    const int *runp = run_table(runs, n_runs, kc, "attn_rows");
    attn_chunk_launch("attn_chunk_rows", "attn_rows", q, q_ld, kc, vc, y,
                      table_rows(rows, batch), runp, n_runs,
                      batch, n_heads0, kv_mul, head_dim, splits, ml_scratch,
                      o_scratch, zq, zs, zbs, k_scales, v_scales);
}

// attn_paged with the rows grouped into runs: every timestep of a run is
// found through the page list of the run's sequence.
void attn_chunk_paged(torch::Tensor q, int64_t q_ld, torch::Tensor kc,
                      torch::Tensor vc, torch::Tensor y, torch::Tensor rows,
                      torch::Tensor page_table, int64_t page_size,
                      torch::Tensor runs, int64_t n_runs, int64_t batch,
                      int64_t n_heads0, int64_t kv_mul, int64_t head_dim,
                      int64_t splits, torch::Tensor ml_scratch,
                      torch::Tensor o_scratch, OptTensor zq = c10::nullopt,
                      OptTensor zs = c10::nullopt, OptTensor zbs = c10::nullopt,
                      OptTensor k_scales = c10::nullopt,
                      OptTensor v_scales = c10::nullopt) {
    const int *runp = run_table(runs, n_runs, kc, "attn_paged");
    TORCH_CHECK(kc.dim() == 2, "attn_chunk_paged: caches are [rows, kv_dim0]");
    attn_chunk_launch("attn_chunk_paged", "attn_paged", q, q_ld, kc, vc, y,
                      paged_rows(rows, page_table, page_size, batch, kc), runp,
                      n_runs, batch, n_heads0, kv_mul, head_dim, splits,
                      ml_scratch, o_scratch, zq, zs, zbs, k_scales, v_scales);
}

// Decode-row attention with the query heads of a KV head packed into the
// MFMA: k_attn_gqa fills the split scratch (any splits >= 1), the combine
// finishes. f16 caches, and int8 (Q80) ones with their scale planes; `other`
// names the binding that serves the rest.
template <typename ROWS>
static void attn_gqa_launch(const char *name, const char *other,
                            torch::Tensor &q, int64_t q_ld, torch::Tensor &kc,
                            torch::Tensor &vc, torch::Tensor &y, ROWS rows,
                            int64_t batch, int64_t n_heads0, int64_t kv_mul,
                            int64_t head_dim, int64_t splits,
                            torch::Tensor &ml_scratch, torch::Tensor &o_scratch,
                            OptTensor &zq, OptTensor &zs, OptTensor &zbs,
                            const OptTensor &k_scales,
                            const OptTensor &v_scales) {
    CHECK_CUDA(q);
    const bool f16 = kc.scalar_type() == at::kHalf
                  && vc.scalar_type() == at::kHalf;
    const bool q80 = kc.scalar_type() == at::kChar
                  && vc.scalar_type() == at::kChar;
    TORCH_CHECK(f16 || q80, name, " serves a float16 or an int8 (Q80) KV "
                "cache: use ", other, " for a float32 cache");
    TORCH_CHECK(q80 || (!k_scales.has_value() && !v_scales.has_value()), name,
                " takes k_scales / v_scales with an int8 (Q80) KV cache only");
    TORCH_CHECK(f16 || (k_scales.has_value() && v_scales.has_value()), name,
                ": an int8 (Q80) KV cache needs k_scales= and v_scales=");
    const KVScales sc = kv_scales(kc, vc, k_scales, v_scales);
    TORCH_CHECK(head_dim == 64 || head_dim == 128, name,
                " serves head_dim 64 and 128 (got ", head_dim, "): use ", other);
    TORCH_CHECK(kv_mul >= 1 && kv_mul <= GQA_HEADS, name, " serves kv_mul 1..",
                GQA_HEADS, " (got ", kv_mul, "): use ", other);
    TORCH_CHECK(n_heads0 % kv_mul == 0, name, ": n_heads0 (", n_heads0,
                ") must be a multiple of kv_mul (", kv_mul, ")");
    TORCH_CHECK(batch >= 1 && splits >= 1 && q_ld % 4 == 0 && kc.dim() == 2
                && kc.is_contiguous() && vc.is_contiguous()
                && kc.sizes() == vc.sizes()
                && kc.size(1) == n_heads0 / kv_mul * head_dim,
                name, ": contiguous caches [rows, n_kv_heads0 * head_dim], "
                "q_ld a multiple of 4");
    const int64_t slots = batch * n_heads0 * splits;
    TORCH_CHECK(ml_scratch.numel() >= slots * 2
                && o_scratch.numel() >= slots * head_dim,
                name, ": split scratch too small for ", slots, " partials");
    const bool quant = zq.has_value();
    float *yp = quant ? nullptr : y.data_ptr<float>();
    int8_t *zqp = quant ? zq->data_ptr<int8_t>() : nullptr;
    float *zsp = quant ? zs->data_ptr<float>() : nullptr;
    float *zbsp = quant ? zbs->data_ptr<float>() : nullptr;
    with_head_vec(head_dim, [&](auto vec_const) {
        constexpr int V = decltype(vec_const)::value;
        with_kv_ptrs(kc, vc, [&](auto *kcp, auto *vcp) {
            using KVT = std::remove_pointer_t<decltype(kcp)>;
            auto launch = [&](auto krows) {
                hipLaunchKernelGGL((k_attn_gqa<V, KVT, decltype(krows)>),
                                   dim3(n_heads0 / kv_mul, batch, splits),
                                   dim3(GQA_NW * WAVE), 0, cur_stream(),
                                   q.data_ptr<float>(), (int)q_ld, kcp, vcp,
                                   krows, (int)n_heads0, (int)kv_mul,
                                   (int)kc.size(1),
                                   1.0f / sqrtf((float)head_dim),
                                   ml_scratch.data_ptr<float>(),
                                   o_scratch.data_ptr<float>());
            };
            if constexpr (kKVQ80<KVT>)
                launch(Q80Rows<ROWS>{rows, sc.k, sc.v});
            else if constexpr (std::is_same_v<KVT, __half>)
                launch(rows);
        });
        combine_launch<V>(ml_scratch, o_scratch, yp, zqp, zsp, zbsp, batch,
                          n_heads0, splits);
    });
}

// attn for decode rows of one sequence: row b is position pos[0]+b.
void attn_gqa(torch::Tensor q, int64_t q_ld, torch::Tensor kc, torch::Tensor vc,
              torch::Tensor y, torch::Tensor pos, int64_t batch,
              int64_t n_heads0, int64_t kv_mul, int64_t head_dim,
              int64_t splits, torch::Tensor ml_scratch, torch::Tensor o_scratch,
              OptTensor zq = c10::nullopt, OptTensor zs = c10::nullopt,
              OptTensor zbs = c10::nullopt, OptTensor k_scales = c10::nullopt,
              OptTensor v_scales = c10::nullopt) {
    attn_gqa_launch("attn_gqa", "attn", q, q_ld, kc, vc, y,
                    SeqRows{pos.data_ptr<int>()}, batch, n_heads0, kv_mul,
                    head_dim, splits, ml_scratch, o_scratch, zq, zs, zbs,
                    k_scales, v_scales);
}

void attn_gqa_rows(torch::Tensor q, int64_t q_ld, torch::Tensor kc,
                   torch::Tensor vc, torch::Tensor y, torch::Tensor rows,
                   int64_t batch, int64_t n_heads0, int64_t kv_mul,
                   int64_t head_dim, int64_t splits, torch::Tensor ml_scratch,
                   torch::Tensor o_scratch, OptTensor zq = c10::nullopt,
                   OptTensor zs = c10::nullopt, OptTensor zbs = c10::nullopt,
                   OptTensor k_scales = c10::nullopt,
                   OptTensor v_scales = c10::nullopt) {
    attn_gqa_launch("attn_gqa_rows", "attn_rows", q, q_ld, kc, vc, y,
                    table_rows(rows, batch), batch, n_heads0, kv_mul, head_dim,
                    splits, ml_scratch, o_scratch, zq, zs, zbs, k_scales,
                    v_scales);
}

void attn_gqa_paged(torch::Tensor q, int64_t q_ld, torch::Tensor kc,
                    torch::Tensor vc, torch::Tensor y, torch::Tensor rows,
                    torch::Tensor page_table, int64_t page_size, int64_t batch,
                    int64_t n_heads0, int64_t kv_mul, int64_t head_dim,
                    int64_t splits, torch::Tensor ml_scratch,
                    torch::Tensor o_scratch, OptTensor zq = c10::nullopt,
                    OptTensor zs = c10::nullopt, OptTensor zbs = c10::nullopt,
                    OptTensor k_scales = c10::nullopt,
                    OptTensor v_scales = c10::nullopt) {
    TORCH_CHECK(kc.dim() == 2, "attn_gqa_paged: caches are [rows, kv_dim0]");
    attn_gqa_launch("attn_gqa_paged", "attn_paged", q, q_ld, kc, vc, y,
                    paged_rows(rows, page_table, page_size, batch, kc), batch,
                    n_heads0, kv_mul, head_dim, splits, ml_scratch, o_scratch,
                    zq, zs, zbs, k_scales, v_scales);
}

// Decode-row attention over a paged cache whose rows share leading pages:
// k_attn_prefix attends every group's common prefix once into the prefix
// scratch (pre_ml / pre_o, S_pre partials per (row, head)), k_attn_gqa over
// SuffixRows attends every row's own rest into the split scratch, and
// k_attn_combine_pre merges the two. The three launches do not depend on the
// tables' contents (models/rows.py prefix_groups builds them; the kernels
// clamp what they read from them): with no live group the first leaves at
// once and the suffix is the whole history.
void attn_prefix_paged(torch::Tensor q, int64_t q_ld, torch::Tensor kc,
                       torch::Tensor vc, torch::Tensor y, torch::Tensor rows,
                       torch::Tensor page_table, int64_t page_size,
                       torch::Tensor pre_rows, torch::Tensor groups,
                       torch::Tensor members, torch::Tensor n_groups_dev,
                       int64_t batch, int64_t n_heads0, int64_t kv_mul,
                       int64_t head_dim, int64_t splits,
                       torch::Tensor ml_scratch, torch::Tensor o_scratch,
                       int64_t pre_splits, torch::Tensor pre_ml,
                       torch::Tensor pre_o, OptTensor zq = c10::nullopt,
                       OptTensor zs = c10::nullopt,
                       OptTensor zbs = c10::nullopt,
                       OptTensor k_scales = c10::nullopt,
                       OptTensor v_scales = c10::nullopt) {
    const char *name = "attn_prefix_paged";
    CHECK_CUDA(q);
    TORCH_CHECK(q.scalar_type() == at::kFloat, name, ": q must be float32");
    TORCH_CHECK(kc.dim() == 2, name, ": caches are [rows, kv_dim0]");
    const bool f16 = kc.scalar_type() == at::kHalf
                  && vc.scalar_type() == at::kHalf;
    const bool q80 = kc.scalar_type() == at::kChar
                  && vc.scalar_type() == at::kChar;
    TORCH_CHECK(f16 || q80, name, " serves a float16 or an int8 (Q80) KV "
                "cache: use attn_paged for a float32 cache");
    TORCH_CHECK(q80 || (!k_scales.has_value() && !v_scales.has_value()), name,
                " takes k_scales / v_scales with an int8 (Q80) KV cache only");
    TORCH_CHECK(f16 || (k_scales.has_value() && v_scales.has_value()), name,
                ": an int8 (Q80) KV cache needs k_scales= and v_scales=");
    const KVScales sc = kv_scales(kc, vc, k_scales, v_scales);
    TORCH_CHECK(head_dim == 64 || head_dim == 128, name,
                " serves head_dim 64 and 128 (got ", head_dim,
                "): use attn_paged");
    TORCH_CHECK(kv_mul >= 1 && kv_mul <= PRE_HEADS, name, " serves kv_mul 1..",
                PRE_HEADS, " (got ", kv_mul, "): use attn_paged");
    TORCH_CHECK(n_heads0 % kv_mul == 0, name, ": n_heads0 (", n_heads0,
                ") must be a multiple of kv_mul (", kv_mul, ")");
    TORCH_CHECK(splits <= 65535 && pre_splits <= 65535 && batch <= 65535, name,
                ": batch, splits and pre_splits are grid dimensions, at most "
                "65535 each");
    TORCH_CHECK(batch >= 1 && splits >= 1 && pre_splits >= 1 && q_ld % 4 == 0
                && kc.is_contiguous() && vc.is_contiguous()
                && kc.sizes() == vc.sizes()
                && kc.size(1) == n_heads0 / kv_mul * head_dim,
                name, ": contiguous caches [rows, n_kv_heads0 * head_dim], "
                "q_ld a multiple of 4");
    const PagedRows paged = paged_rows(rows, page_table, page_size, batch, kc);
    auto int_table = [&](const torch::Tensor &t, const char *what) {
        CHECK_CUDA(t);
        TORCH_CHECK(t.scalar_type() == at::kInt && t.is_contiguous()
                    && t.device() == kc.device(), name, ": ", what,
                    " must be a contiguous int32 tensor on the cache's device");
    };
    int_table(pre_rows, "pre_rows");
    int_table(groups, "groups");
    int_table(members, "members");
    int_table(n_groups_dev, "n_groups_dev");
    TORCH_CHECK(pre_rows.dim() == 2 && pre_rows.size(1) == 2
                && pre_rows.size(0) >= batch, name,
                ": pre_rows must be int32 [>= batch, 2]");
    TORCH_CHECK(groups.dim() == 2 && groups.size(1) == 2
                && groups.size(0) >= 1 && groups.size(0) <= 65535, name,
                ": groups must be int32 [1..65535, 2]");
    TORCH_CHECK(members.numel() >= 1 && n_groups_dev.numel() >= 1, name,
                ": members and n_groups_dev must not be empty");
    const int64_t slots = batch * n_heads0 * splits;
    TORCH_CHECK(ml_scratch.numel() >= slots * 2
                && o_scratch.numel() >= slots * head_dim,
                name, ": split scratch too small for ", slots, " partials");
    const int64_t pslots = batch * n_heads0 * pre_splits;
    TORCH_CHECK(pre_ml.numel() >= pslots * 2
                && pre_o.numel() >= pslots * head_dim,
                name, ": prefix scratch too small for ", pslots, " partials");
    for (const torch::Tensor *t : {&ml_scratch, &o_scratch, &pre_ml, &pre_o})
        TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous()
                    && t->device() == kc.device(), name,
                    ": scratch must be contiguous float32 on the cache's device");
    const bool quant = zq.has_value();
    float *yp = quant ? nullptr : y.data_ptr<float>();
    int8_t *zqp = quant ? zq->data_ptr<int8_t>() : nullptr;
    float *zsp = quant ? zs->data_ptr<float>() : nullptr;
    float *zbsp = quant ? zbs->data_ptr<float>() : nullptr;
    const int kv_dim0 = kc.size(1);
    const float scale = 1.0f / sqrtf((float)head_dim);
    const int n_kv = n_heads0 / kv_mul;
    const SuffixRows suffix{paged, pre_rows.data_ptr<int>()};
    with_head_vec(head_dim, [&](auto vec_const) {
        constexpr int V = decltype(vec_const)::value;
        with_kv_ptrs(kc, vc, [&](auto *kcp, auto *vcp) {
            using KVT = std::remove_pointer_t<decltype(kcp)>;
            auto launch = [&](auto prows, auto srows) {
                hipLaunchKernelGGL((k_attn_prefix<V, KVT, decltype(prows)>),
                                   dim3(n_kv, groups.size(0), pre_splits),
                                   dim3(PRE_NW * WAVE), 0, cur_stream(),
                                   q.data_ptr<float>(), (int)q_ld, kcp, vcp,
                                   prows, pre_rows.data_ptr<int>(),
                                   groups.data_ptr<int>(),
                                   members.data_ptr<int>(),
                                   (int)members.numel(),
                                   n_groups_dev.data_ptr<int>(), (int)batch,
                                   (int)n_heads0, (int)kv_mul, kv_dim0, scale,
                                   pre_ml.data_ptr<float>(),
                                   pre_o.data_ptr<float>());
                hipLaunchKernelGGL((k_attn_gqa<V, KVT, decltype(srows)>),
                                   dim3(n_kv, batch, splits),
                                   dim3(GQA_NW * WAVE), 0, cur_stream(),
                                   q.data_ptr<float>(), (int)q_ld, kcp, vcp,
                                   srows, (int)n_heads0, (int)kv_mul, kv_dim0,
                                   scale, ml_scratch.data_ptr<float>(),
                                   o_scratch.data_ptr<float>());
            };
            if constexpr (kKVQ80<KVT>)
                launch(Q80Rows<PagedRows>{paged, sc.k, sc.v},
                       Q80Rows<SuffixRows>{suffix, sc.k, sc.v});
            else if constexpr (std::is_same_v<KVT, __half>)
                launch(paged, suffix);
        });
        auto combine = [&](auto quant_const) {
            hipLaunchKernelGGL(
                (k_attn_combine_pre<V, decltype(quant_const)::value>),
                dim3(n_heads0, batch), dim3(V * WAVE), 0, cur_stream(),
                ml_scratch.data_ptr<float>(), o_scratch.data_ptr<float>(),
                pre_ml.data_ptr<float>(), pre_o.data_ptr<float>(),
                pre_rows.data_ptr<int>(), yp, zqp, zsp, zbsp, (int)n_heads0,
                (int)splits, (int)pre_splits);
        };
        if (zqp) combine(std::true_type{});
        else combine(std::false_type{});
    });
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
    m.def("attn_chunk", &attn_chunk, py::arg("q"), py::arg("q_ld"),
          py::arg("kc"), py::arg("vc"), py::arg("y"), py::arg("pos"),
          py::arg("batch"), py::arg("n_heads0"), py::arg("kv_mul"),
          py::arg("head_dim"), py::arg("splits"), py::arg("ml_scratch"),
          py::arg("o_scratch"), py::arg("zq") = py::none(),
          py::arg("zs") = py::none(), py::arg("zbs") = py::none(),
          KV_SCALE_ARGS);
    m.def("attn_chunk_rows", &attn_chunk_rows, py::arg("q"), py::arg("q_ld"),
          py::arg("kc"), py::arg("vc"), py::arg("y"), py::arg("rows"),
          py::arg("runs"), py::arg("n_runs"), py::arg("batch"),
          py::arg("n_heads0"), py::arg("kv_mul"), py::arg("head_dim"),
          py::arg("splits"), py::arg("ml_scratch"), py::arg("o_scratch"),
          py::arg("zq") = py::none(), py::arg("zs") = py::none(),
          py::arg("zbs") = py::none(), KV_SCALE_ARGS);
    m.def("attn_chunk_paged", &attn_chunk_paged, py::arg("q"), py::arg("q_ld"),
          py::arg("kc"), py::arg("vc"), py::arg("y"), py::arg("rows"),
          py::arg("page_table"), py::arg("page_size"), py::arg("runs"),
          py::arg("n_runs"), py::arg("batch"), py::arg("n_heads0"),
          py::arg("kv_mul"), py::arg("head_dim"), py::arg("splits"),
          py::arg("ml_scratch"), py::arg("o_scratch"),
          py::arg("zq") = py::none(), py::arg("zs") = py::none(),
          py::arg("zbs") = py::none(), KV_SCALE_ARGS);
    m.def("attn_chunk_wide", &attn_chunk_wide, py::arg("q"), py::arg("q_ld"),
          py::arg("kc"), py::arg("vc"), py::arg("y"), py::arg("pos"),
          py::arg("batch"), py::arg("n_heads0"), py::arg("kv_mul"),
          py::arg("head_dim"), py::arg("splits"), py::arg("ml_scratch"),
          py::arg("o_scratch"), py::arg("zq") = py::none(),
          py::arg("zs") = py::none(), py::arg("zbs") = py::none(),
          KV_SCALE_ARGS);
    m.def("attn_gqa", &attn_gqa, py::arg("q"), py::arg("q_ld"), py::arg("kc"),
          py::arg("vc"), py::arg("y"), py::arg("pos"), py::arg("batch"),
          py::arg("n_heads0"), py::arg("kv_mul"), py::arg("head_dim"),
          py::arg("splits"), py::arg("ml_scratch"), py::arg("o_scratch"),
          py::arg("zq") = py::none(), py::arg("zs") = py::none(),
          py::arg("zbs") = py::none(), KV_SCALE_ARGS);
    m.def("attn_gqa_rows", &attn_gqa_rows, py::arg("q"), py::arg("q_ld"),
          py::arg("kc"), py::arg("vc"), py::arg("y"), py::arg("rows"),
          py::arg("batch"), py::arg("n_heads0"), py::arg("kv_mul"),
          py::arg("head_dim"), py::arg("splits"), py::arg("ml_scratch"),
          py::arg("o_scratch"), py::arg("zq") = py::none(),
          py::arg("zs") = py::none(), py::arg("zbs") = py::none(),
          KV_SCALE_ARGS);
    m.def("attn_gqa_paged", &attn_gqa_paged, py::arg("q"), py::arg("q_ld"),
          py::arg("kc"), py::arg("vc"), py::arg("y"), py::arg("rows"),
          py::arg("page_table"), py::arg("page_size"), py::arg("batch"),
          py::arg("n_heads0"), py::arg("kv_mul"), py::arg("head_dim"),
          py::arg("splits"), py::arg("ml_scratch"), py::arg("o_scratch"),
          py::arg("zq") = py::none(), py::arg("zs") = py::none(),
          py::arg("zbs") = py::none(), KV_SCALE_ARGS);
    m.def("attn_prefix_paged", &attn_prefix_paged, py::arg("q"),
          py::arg("q_ld"), py::arg("kc"), py::arg("vc"), py::arg("y"),
          py::arg("rows"), py::arg("page_table"), py::arg("page_size"),
          py::arg("pre_rows"), py::arg("groups"), py::arg("members"),
          py::arg("n_groups_dev"), py::arg("batch"), py::arg("n_heads0"),
          py::arg("kv_mul"), py::arg("head_dim"), py::arg("splits"),
          py::arg("ml_scratch"), py::arg("o_scratch"), py::arg("pre_splits"),
          py::arg("pre_ml"), py::arg("pre_o"), py::arg("zq") = py::none(),
          py::arg("zs") = py::none(), py::arg("zbs") = py::none(),
          KV_SCALE_ARGS);
    m.def("kv_append", &kv_append);
    m.def("attn", &attn, py::arg("q"), py::arg("q_ld"), py::arg("kc"), py::arg("vc"),
          py::arg("y"), py::arg("pos"), py::arg("batch"), py::arg("n_heads0"),
          py::arg("kv_mul"), py::arg("head_dim"), py::arg("splits"),
          py::arg("ml_scratch"), py::arg("o_scratch"), py::arg("counter"),
          py::arg("zq") = py::none(), py::arg("zs") = py::none(),
          py::arg("zbs") = py::none(), KV_SCALE_ARGS);
}
