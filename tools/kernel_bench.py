"""Per-kernel microbench on Llama-3.1-8B decode shapes (isolated graphs)."""
import os, statistics, sys, time, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dllama_amd.ops import hip_ops

k = hip_ops()
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)

def bench(fn, n=256, reps=10):
    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3): fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(n): fn()
    for _ in range(3): gr.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps): gr.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps / n * 1e6

def attn_ab(positions=(32, 128, 250, 500, 1000), rounds=5):
    """Short-context attention alone in an isolated hipGraph at 8B shapes
    (32 heads, kv_mul 4, hd 128, f16 KV, Q80 output): the split + combine
    pair at S=8 and S=16 against the single S=1 launch. S=1 is the wide
    16-wave kernel in this tree; run this file from a checkout of an older
    commit to time the 4-wave fused kernel it replaced. The candidates are
    interleaved over `rounds`; median and min us per call.

      python tools/kernel_bench.py attn     this section alone"""
    H0, hd, kvd, seq, kv_mul = 32, 128, 1024, 2048, 4
    kc = (torch.randn(seq, kvd, device=dev, generator=g) * 0.3).half()
    vc = torch.randn(seq, kvd, device=dev, generator=g).half()
    qv = torch.randn(1, H0 * hd, device=dev, generator=g)
    y = torch.zeros(1, H0 * hd, device=dev)
    zq = torch.zeros(1, H0 * hd, dtype=torch.int8, device=dev)
    zs = torch.zeros(1, H0 * hd // 32, device=dev)
    zbs = torch.zeros(1, H0 * hd // 32, device=dev)
    cnt = torch.zeros(H0, dtype=torch.int32, device=dev)
    cands = (("pair S=8", 8), ("pair S=16", 16), ("single S=1", 1))
    scr = {S: (torch.zeros(H0 * S * 2, device=dev),
               torch.zeros(H0 * S * hd, device=dev)) for _, S in cands}
    print("\n-- attention, isolated graph, 8B shapes, f16 KV, Q80 out "
          "(us per call: median / min) --")
    for p in positions:
        pos = torch.tensor([p], dtype=torch.int32, device=dev)
        times = {name: [] for name, _ in cands}
        for _ in range(rounds):
            for name, S in cands:
                ml, osc = scr[S]
                times[name].append(bench(
                    lambda: k.attn(qv, H0 * hd, kc, vc, y, pos, 1, H0, kv_mul,
                                   hd, S, ml, osc, cnt, zq, zs, zbs),
                    n=128, reps=5))
        print(f"pos={p:5d}  " + "  ".join(
            f"{name}: {statistics.median(t):6.2f} / {min(t):6.2f}"
            for name, t in times.items()))


def resid_ab(rounds=5, forms=(16, 8, 4)):
    """q40_gemv_resid_q alone in an isolated hipGraph at the down-projection
    shapes (wo, w2) of the 1B, 3B, 8B and 70B presets, one column per
    workgroup form: 16 waves (the block assembled in one workgroup's LDS)
    and the 8- and 4-wave hand-off forms (last arriver emits the block),
    forced through q40_gemv_resid_q_waves(). The forms are interleaved over
    `rounds`; median / min us per call. Two figures per form:

      hbm    the graph rotates over distinct weight copies that together
             exceed 300 MB, more than the 256 MiB Infinity Cache holds, so
             every launch streams its matrix from HBM as a decode step does
      cache  one matrix replayed 64 times, served by the Infinity Cache

      python tools/kernel_bench.py resid     this section alone"""
    shapes = []
    for tag, dim, ff in (("1b", 2048, 8192), ("3b", 3072, 8192),
                         ("8b", 4096, 14336), ("70b", 8192, 28672)):
        shapes += [(f"{tag} wo", dim, dim), (f"{tag} w2", dim, ff)]
    print("\n-- q40_gemv_resid_q, isolated graph (us per call: median / min); "
          "hbm = rotating >300 MB of weight copies, cache = one matrix --")
    for tag, d, n in shapes:
        nbytes = d * n * 0.5625
        copies = int(300e6 // nbytes) + 1
        qs = torch.randint(0, 256, (copies, d, n // 2), dtype=torch.uint8,
                           device=dev, generator=g)
        sc = (torch.rand((copies, d, n // 32), device=dev, generator=g)
              * 0.01).to(torch.float16)
        xq = torch.randint(-100, 100, (1, n), dtype=torch.int8, device=dev,
                           generator=g)
        xs = torch.rand(1, n // 32, device=dev, generator=g) * 0.01
        xbs = torch.rand(1, n // 32, device=dev, generator=g)
        xr = torch.zeros(1, d, device=dev)
        sq = torch.zeros(16 * 32, device=dev)
        wn = torch.rand(d, device=dev, generator=g)
        oq = torch.zeros(1, d, dtype=torch.int8, device=dev)
        os_ = torch.zeros(1, d // 32, device=dev)
        obs = torch.zeros(1, d // 32, device=dev)
        it = [0]

        def rotating():
            i = it[0] % copies
            it[0] += 1
            k.q40_gemv_resid_q(qs[i], sc[i], xq, xs, xbs, xr, sq, wn, oq, os_, obs)

        def single():
            k.q40_gemv_resid_q(qs[0], sc[0], xq, xs, xbs, xr, sq, wn, oq, os_, obs)

        nrot = max(64, copies)
        times = {(f, v): [] for f in forms for v in ("hbm", "cache")}
        for _ in range(rounds):
            for f in forms:
                k.q40_gemv_resid_q_waves(f)
                it[0] = 0
                times[(f, "hbm")].append(bench(rotating, n=nrot, reps=5))
                times[(f, "cache")].append(bench(single, n=64, reps=5))
        k.q40_gemv_resid_q_waves(0)
        ideal = nbytes / 6.3e3 / 1000  # us at 6.3 TB/s
        print(f"{tag:7s} {d:5d}x{n:<5d} {nbytes / 1e6:6.1f} MB x{copies:<3d} "
              f"ideal {ideal:5.2f} | " + " | ".join(
                  f"{f:2d}w hbm {statistics.median(times[(f, 'hbm')]):6.2f} /"
                  f" {min(times[(f, 'hbm')]):6.2f}"
                  f" cache {statistics.median(times[(f, 'cache')]):6.2f} /"
                  f" {min(times[(f, 'cache')]):6.2f}" for f in forms))
        del qs, sc


if sys.argv[1:] == ["attn"]:
    attn_ab()
    sys.exit(0)
if sys.argv[1:] == ["resid"]:
    resid_ab()
    sys.exit(0)


def mklin(d, n):
    qs = torch.randint(0, 256, (d, n // 2), dtype=torch.uint8, device=dev, generator=g)
    sc = (torch.rand((d, n // 32), device=dev, generator=g) * 0.01).to(torch.float16)
    return qs, sc

def mkx(nb, n):
    q = torch.randint(-100, 100, (nb, n), dtype=torch.int8, device=dev, generator=g)
    s = torch.rand(nb, n // 32, device=dev, generator=g) * 0.01
    bs = torch.rand(nb, n // 32, device=dev, generator=g)
    return q, s, bs

NB = 1
dim, ffd, qkvd = 4096, 14336, 6144
x = torch.randn(32, dim, device=dev, generator=g)
w = torch.rand(dim, device=dev, generator=g)
ssq = torch.rand(32, 16, device=dev, generator=g) * 100

for d, n, tag in ((4096, 4096, "wo  4096x4096"), (4096, 14336, "w2  4096x14336"),
                  (6144, 4096, "qkv 6144x4096"), (28672, 4096, "w13 28672x4096"),
                  (128256, 4096, "cls 128256x4096")):
    qs, sc = mklin(d, n)
    xq, xs, xbs = mkx(NB, n)
    y = torch.zeros(NB, d, device=dev)
    t_plain = bench(lambda: k.q40_gemv(qs, sc, xq, xs, xbs, y, NB), n=64)
    ideal = (d * n * 0.5625) / 6.3e3 / 1000  # us at 6.3 TB/s
    extra = ""
    if d == dim:
        xr = torch.randn(NB, d, device=dev, generator=g)
        t_resid = bench(lambda: k.q40_gemv_resid(qs, sc, xq, xs, xbs, xr, ssq[0], NB), n=64)
        extra = f" resid={t_resid:6.2f}us"
    print(f"{tag:16s} plain={t_plain:7.2f}us ideal={ideal:6.2f}us eff={100*ideal/t_plain:4.0f}%{extra}")

# norm / small kernels at decode shapes
q8 = torch.zeros(1, dim, dtype=torch.int8, device=dev)
s8 = torch.zeros(1, dim // 32, device=dev)
bs8 = torch.zeros(1, dim // 32, device=dev)
print("norm_quant  [1,4096]: %6.2f us" % bench(lambda: k.norm_quant(x[:1], w, ssq, q8, s8, bs8, 1, 1e-5)))
ff = torch.randn(1, 2 * ffd, device=dev, generator=g)
dq = torch.zeros(1, ffd, dtype=torch.int8, device=dev)
ds = torch.zeros(1, ffd // 32, device=dev)
dbs = torch.zeros(1, ffd // 32, device=dev)
print("swiglu_q80  [1,14336]: %6.2f us" % bench(lambda: k.swiglu_q80(ff, ff[:, ffd:], 2 * ffd, ffd, 1, dq, ds, dbs)))

# attention decode at pos=1024, 8B shapes
H0, hd, kvd, seq = 32, 128, 1024, 4096
kc = torch.randn(seq, kvd, device=dev, generator=g)
vc = torch.randn(seq, kvd, device=dev, generator=g)
qv = torch.randn(1, H0 * hd, device=dev, generator=g)
z = torch.zeros(1, H0 * hd, device=dev)
pos = torch.tensor([1024], dtype=torch.int32, device=dev)
S = 32
ml = torch.zeros(1 * H0 * S * 2, device=dev)
osc = torch.zeros(1 * H0 * S * hd, device=dev)
cnt = torch.zeros(1 * H0, dtype=torch.int32, device=dev)
zq3 = mkx(1, H0 * hd)
print("attn(pos=1024) fused+quant: %6.2f us" %
      bench(lambda: k.attn(qv, H0 * hd, kc, vc, z, pos, 1, H0, 4, hd, S, ml, osc,
                           cnt, zq3[0], zq3[1], zq3[2])))
pos2 = torch.tensor([64], dtype=torch.int32, device=dev)
print("attn(pos=64)  fused+quant: %6.2f us" %
      bench(lambda: k.attn(qv, H0 * hd, kc, vc, z, pos2, 1, H0, 4, hd, S, ml, osc,
                           cnt, zq3[0], zq3[1], zq3[2])))
xr = torch.randn(1, dim, device=dev, generator=g)
pr = torch.randn(1, dim, device=dev, generator=g)
print("add_ssq [1,4096]: %6.2f us" % bench(lambda: k.add_ssq(xr, pr, ssq[0], 1)))

# separate norm_quant + gemv, NB=1
for d, n, tag in ((6144, 4096, "qkv"), (28672, 4096, "w13"), (128256, 4096, "cls")):
    qs, sc = mklin(d, n)
    xq, xs, xbs = mkx(1, n)
    y = torch.zeros(1, d, device=dev)
    q8b = torch.zeros(1, n, dtype=torch.int8, device=dev)
    s8b = torch.zeros(1, n // 32, device=dev)
    bs8b = torch.zeros(1, n // 32, device=dev)
    wn = torch.rand(n, device=dev, generator=g)
    xf = torch.randn(1, n, device=dev, generator=g)
    sq = torch.rand(1, 16 * 32, device=dev, generator=g)
    def sep():
        k.norm_quant(xf, wn, sq, q8b, s8b, bs8b, 1, 1e-5)
        k.q40_gemv(qs, sc, q8b, s8b, bs8b, y, 1)
    t_sep = bench(sep, n=64)
    print(f"{tag:4s}: norm_quant+gemv={t_sep:6.2f}us")

# prefill GEMM v1 vs v2 (round-2 DLLAMA_GEMM_V2 candidate), batch 32
print("\n-- GEMM v1 vs v2 (batch 32) --")
part = torch.zeros(16 * 32 * 28672, device=dev)
for d, n, tag in ((6144, 4096, "qkv"), (4096, 14336, "w2"), (28672, 4096, "w13")):
    qs, sc = mklin(d, n)
    xq, xs, _ = mkx(32, n)
    y = torch.zeros(32, d, device=dev)
    t1 = bench(lambda: k.q40_gemm(qs, sc, xq, xs, y, 32, part, variant=0), n=32)
    t2 = bench(lambda: k.q40_gemm(qs, sc, xq, xs, y, 32, part, variant=1), n=32)
    ideal = (d * n * 0.5625) / 6.3e3 / 1000
    print(f"gemm {tag:4s} v1={t1:7.2f}us v2={t2:7.2f}us ideal={ideal:6.2f}us "
          f"v2-eff={100*ideal/t2:4.0f}%")

# grouped GEMV v1 vs v2 at Qwen3-30B-A3B decode shapes
print("\n-- grouped GEMV v1 vs v2 (qwen3-30b shapes, 8 slots) --")
for d, n, ks, tag in ((1536, 2048, 8, "w13"), (2048, 768, 1, "w2")):
    E = 16
    qs = torch.randint(0, 256, (E, d, n // 2), dtype=torch.uint8, device=dev, generator=g)
    sc = (torch.rand((E, d, n // 32), device=dev, generator=g) * 0.01).to(torch.float16)
    nx = 8 // ks
    xq, xs, xbs = mkx(max(1, nx), n)
    idx = torch.arange(8, dtype=torch.int32, device=dev) % E
    y = torch.zeros(8, d, device=dev)
    t1 = bench(lambda: k.q40_gemv_grouped(qs, sc, xq, xs, xbs, idx, y, ks, variant=0), n=64)
    t2 = bench(lambda: k.q40_gemv_grouped(qs, sc, xq, xs, xbs, idx, y, ks, variant=1), n=64)
    ideal = (8 * d * n * 0.5625) / 6.3e3 / 1000
    print(f"grouped {tag:4s} v1={t1:7.2f}us v2={t2:7.2f}us ideal={ideal:6.2f}us "
          f"v2-eff={100*ideal/t2:4.0f}%")

attn_ab()
resid_ab()
