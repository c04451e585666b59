// dllama_amd — host-only code: the CPU Q40 matmul and the native BPE encoder.

#if defined(__AVX2__)
#include <immintrin.h>
#endif
#include <vector>
#include <thread>
#if defined(_OPENMP)
#include <omp.h>
#endif
#include "dllama_common.h"

// ------------------------------------------------------------ CPU Q40 GEMM
// Native CPU matmul streaming Q40 planes directly (no f32 dequant copy):
// y[b, row] = sum_blk scale * sum_k (q-8) * x — keeps CPU serving at
// quantized-weight RAM (role of the reference's AVX512/NEON CPU kernels,
// src/nn/nn-cpu-ops.cpp:231-449). Parallel over rows via at::parallel_for
// (torch threads, the CLI's --nthreads). The inner 32-wide block loop
// auto-vectorizes; activations stay f32 (more precise than the reference's
// Q80 activations, same wire format compatibility).
void q40_matmul_cpu(torch::Tensor qs, torch::Tensor scales, torch::Tensor x,
                    torch::Tensor y) {
    TORCH_CHECK(!qs.is_cuda() && !x.is_cuda(), "q40_matmul_cpu is CPU-only");
    CHECK_CONT(qs); CHECK_CONT(x);
    const int d = qs.size(0);
    const int n = qs.size(1) * 2;
    const int B = x.size(0);
    const int nb = n / QB;
    TORCH_CHECK(x.size(-1) == n, "x width mismatch");
    const uint8_t *W = qs.data_ptr<uint8_t>();
    const at::Half *S = scales.data_ptr<at::Half>();
    const float *X = x.data_ptr<float>();
    float *Y = y.data_ptr<float>();
    // Q80-quantize the activations once (the same per-32-block wire the GPU
    // path and the reference use, nn-quants.cpp:67), then int8 block dots —
    // 8-bit integer MACs are what x86 actually vectorizes for this format
    // (role of the reference's AVX2/AVX512 matmul, nn-cpu-ops.cpp:231-449).
    std::vector<int8_t> xq((size_t)B * n);
    std::vector<float> xsc((size_t)B * nb), xbs((size_t)B * nb);
    for (int b = 0; b < B; b++) {
        const float *xr = X + (int64_t)b * n;
        for (int blk = 0; blk < nb; blk++) {
            float amax = 0.0f;
            for (int j = 0; j < QB; j++)
                amax = std::max(amax, std::fabs(xr[blk * QB + j]));
            const float dd = amax / 127.0f;
            const float qinv = dd > 0.0f ? 1.0f / dd : 0.0f;
            float bsum = 0.0f;
            for (int j = 0; j < QB; j++) {
                const float qf = std::rint(xr[blk * QB + j] * qinv);
                xq[(size_t)b * n + blk * QB + j] = (int8_t)qf;
                bsum += qf;
            }
            xsc[(size_t)b * nb + blk] = dd;
            xbs[(size_t)b * nb + blk] = bsum;
        }
    }
    // OpenMP over rows: at::parallel_for silently serialized here (measured
    // 1-thread == 8-thread) and per-call std::thread spawn costs ~0.3 ms;
    // omp's persistent pool respects torch's thread count via num_threads.
    // blocktime MUST be short: libomp's default 200 ms post-region spin
    // starves torch's own intra-op pool between our regions (measured
    // 61 s/token on a 256-core box); 1 ms still covers back-to-back
    // matmuls. Capped at 64 threads — the op is memory-bound.
#if defined(_OPENMP)
    static const bool _bt0 = [] { kmp_set_blocktime(1); return true; }();
    (void)_bt0;
#endif
    const int nt = std::min(64, std::max(1, (int)at::get_num_threads()));
    auto worker = [&](int64_t r0, int64_t r1) {
        for (int64_t row = r0; row < r1; row++) {
            const uint8_t *w = W + row * (n >> 1);
            const at::Half *sc = S + row * nb;
            for (int b = 0; b < B; b++) {
                const int8_t *xr = xq.data() + (size_t)b * n;
                const float *sx = xsc.data() + (size_t)b * nb;
                const float *bs = xbs.data() + (size_t)b * nb;
                float acc = 0.0f;
#if defined(__AVX2__)
                const __m128i m0f = _mm_set1_epi8(0x0F);
                const __m256i ones = _mm256_set1_epi16(1);
                for (int blk = 0; blk < nb; blk++) {
                    const __m128i raw = _mm_loadu_si128(
                        reinterpret_cast<const __m128i *>(w + blk * 16));
                    const __m128i lo = _mm_and_si128(raw, m0f);
                    const __m128i hi = _mm_and_si128(_mm_srli_epi16(raw, 4), m0f);
                    const __m256i w8 = _mm256_set_m128i(hi, lo);  // u8 in 0..15
                    const __m256i x8 = _mm256_loadu_si256(
                        reinterpret_cast<const __m256i *>(xr + blk * QB));
                    // u8*i8 pair-sums (|pair| <= 2*15*127 < 2^15: no saturation)
                    const __m256i p16 = _mm256_maddubs_epi16(w8, x8);
                    const __m256i p32 = _mm256_madd_epi16(p16, ones);
                    __m128i h = _mm_add_epi32(_mm256_castsi256_si128(p32),
                                              _mm256_extracti128_si256(p32, 1));
                    h = _mm_add_epi32(h, _mm_shuffle_epi32(h, 0x4E));
                    h = _mm_add_epi32(h, _mm_shuffle_epi32(h, 0xB1));
                    const int idot = _mm_cvtsi128_si32(h);
                    acc += (float)sc[blk] * sx[blk]
                           * ((float)idot - 8.0f * bs[blk]);
                }
#else
                for (int blk = 0; blk < nb; blk++) {
                    const uint8_t *wb = w + blk * 16;
                    const int8_t *xb = xr + blk * QB;
                    int idot = 0;
                    for (int k = 0; k < 16; k++) {
                        idot += (int)(wb[k] & 15) * xb[k]
                              + (int)(wb[k] >> 4) * xb[k + 16];
                    }
                    acc += (float)sc[blk] * sx[blk]
                           * ((float)idot - 8.0f * bs[blk]);
                }
#endif
                Y[(int64_t)b * d + row] = acc;
            }
        }
    };
    if (nt <= 1 || d < 256) {
        worker(0, d);
    } else {
#if defined(_OPENMP)
        #pragma omp parallel num_threads(nt)
        {
            const int t = omp_get_thread_num();
            const int tn = omp_get_num_threads();
            const int64_t chunk = (d + tn - 1) / tn;
            const int64_t r0 = (int64_t)t * chunk;
            if (r0 < d) worker(r0, std::min<int64_t>(d, r0 + chunk));
        }
#else
        std::vector<std::thread> threads;
        const int64_t chunk = (d + nt - 1) / nt;
        for (int t = 0; t < nt; t++) {
            const int64_t r0 = t * chunk;
            if (r0 >= d) break;
            threads.emplace_back(worker, r0, std::min<int64_t>(d, r0 + chunk));
        }
        for (auto &th : threads) th.join();
#endif
    }
}

// ===================================================== native BPE encoder
// Host-side tokenizer encode (the reference's tokenizer is native C++,
// src/tokenizer.cpp:311-390): exact-match byte accumulation with special
// token scan, then greedy highest-score pair merging. The Python Tokenizer
// delegates here when the extension is loaded.
#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

struct BpeEncoder {
    std::vector<std::string> vocab;
    std::vector<float> scores;
    std::unordered_map<std::string, int> regular;  // first-id wins
    std::vector<int> special_ids;                  // ids >= regular_size
    int regular_size;

    BpeEncoder(const std::vector<std::string> &vocab_,
               const std::vector<double> &scores_, int64_t regular_size_)
        : vocab(vocab_), regular_size((int)regular_size_) {
        scores.reserve(scores_.size());
        for (double s : scores_) scores.push_back((float)s);
        for (int i = 0; i < regular_size && i < (int)vocab.size(); i++)
            regular.emplace(vocab[i], i);  // emplace keeps the first id
        for (int i = regular_size; i < (int)vocab.size(); i++)
            special_ids.push_back(i);
    }

    std::vector<int> encode(const std::string &data, bool add_special) const {
        std::vector<int> tokens;
        std::string buf;
        size_t i = 0;
        while (i < data.size()) {
            if (add_special) {
                int sp = -1;
                for (int sid : special_ids) {
                    const std::string &p = vocab[sid];
                    if (!p.empty() && data.compare(i, p.size(), p) == 0) {
                        sp = sid;
                        break;
                    }
                }
                if (sp >= 0) {
                    if (!buf.empty())
                        throw std::runtime_error("unencodable byte run before special");
                    tokens.push_back(sp);
                    i += vocab[sp].size();
                    continue;
                }
            }
            buf.push_back(data[i++]);
            auto it = regular.find(buf);
            if (it != regular.end()) {
                tokens.push_back(it->second);
                buf.clear();
            }
        }
        if (!buf.empty())
            throw std::runtime_error("cannot encode byte run");

        // greedy merge: globally best-score adjacent pair each round with
        // leftmost tie-break — identical semantics to the reference's O(n^2)
        // rescan (tokenizer.cpp:352-379) via heap + linked list + lazy
        // invalidation (O(n log n)).
        const int n = (int)tokens.size();
        if (n == 0) return tokens;
        std::vector<int> tok(tokens), prev(n), next(n), ver(n, 0);
        for (int j = 0; j < n; j++) { prev[j] = j - 1; next[j] = j + 1 < n ? j + 1 : -1; }
        struct Cand { float score; int pos, id, vl, vr, right; };
        auto worse = [](const Cand &a, const Cand &b) {
            if (a.score != b.score) return a.score < b.score;  // max-heap
            return a.pos > b.pos;                              // leftmost wins
        };
        std::vector<Cand> heap;
        auto push_pair = [&](int l) {
            const int r = next[l];
            if (l < 0 || r < 0) return;
            auto it = regular.find(vocab[tok[l]] + vocab[tok[r]]);
            if (it == regular.end()) return;
            heap.push_back({scores[it->second], l, it->second, ver[l], ver[r], r});
            std::push_heap(heap.begin(), heap.end(), worse);
        };
        for (int j = 0; j + 1 < n; j++) push_pair(j);
        while (!heap.empty()) {
            std::pop_heap(heap.begin(), heap.end(), worse);
            const Cand c = heap.back();
            heap.pop_back();
            const int l = c.pos, r = c.right;
            if (ver[l] != c.vl || ver[r] != c.vr || next[l] != r) continue;
            tok[l] = c.id;
            ver[l]++;
            ver[r]++;
            next[l] = next[r];
            if (next[r] >= 0) prev[next[r]] = l;
            push_pair(prev[l] >= 0 ? prev[l] : -1);
            push_pair(l);
        }
        std::vector<int> out;
        for (int j = 0; j >= 0; j = next[j]) out.push_back(tok[j]);
        return out;
    }
};

void register_host(py::module &m) {
    py::class_<BpeEncoder>(m, "BpeEncoder")
        .def(py::init<const std::vector<std::string> &,
                      const std::vector<double> &, int64_t>())
        .def("encode", [](const BpeEncoder &e, const py::bytes &data,
                          bool add_special) {
            return e.encode(std::string(data), add_special);
        });
    m.def("q40_matmul_cpu", &q40_matmul_cpu);
}
