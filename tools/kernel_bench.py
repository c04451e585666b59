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


def chunk_ab(positions=(512, 2048, 4096, 8192), batches=(32,), rounds=3,
             splits=(8, 16, 32, 64)):
    """Prompt-chunk attention alone in an isolated hipGraph at the 8B shape
    (32 heads, kv_mul 4, hd 128, f16 KV, Q80 output), B rows at first position
    p: k_attn_split + combine against k_attn_chunk + combine at every S,
    interleaved over `rounds`; median us per call, and the largest |code|
    difference between the two Q80 outputs at the first S.

      python tools/kernel_bench.py chunk            B = 32
      python tools/kernel_bench.py chunk-rows       B = 4, 8, 16, 32 (threshold)"""
    H0, hd, kvd, kv_mul = 32, 128, 1024, 4
    seq = max(positions) + 64
    kc = (torch.randn(seq, kvd, device=dev, generator=g) * 0.3).half()
    vc = torch.randn(seq, kvd, device=dev, generator=g).half()
    print("\n-- chunk attention, isolated graph, 8B shape, f16 KV, Q80 out "
          "(median us per call: split / chunk) --")
    for B in batches:
        qv = torch.randn(B, H0 * hd, device=dev, generator=g)
        y = torch.zeros(B, H0 * hd, device=dev)
        cnt = torch.zeros(B * H0, dtype=torch.int32, device=dev)
        z = [[torch.zeros(B, H0 * hd, dtype=torch.int8, device=dev),
              torch.zeros(B, H0 * hd // 32, device=dev),
              torch.zeros(B, H0 * hd // 32, device=dev)] for _ in range(2)]
        for p in positions:
            pos = torch.tensor([p], dtype=torch.int32, device=dev)
            out = []
            for S in splits:
                ml = torch.zeros(B * H0 * S * 2, device=dev)
                osc = torch.zeros(B * H0 * S * hd, device=dev)
                split = lambda: k.attn(qv, H0 * hd, kc, vc, y, pos, B, H0,
                                       kv_mul, hd, S, ml, osc, cnt, *z[0])
                chunk = lambda: k.attn_chunk(qv, H0 * hd, kc, vc, y, pos, B,
                                             H0, kv_mul, hd, S, ml, osc, *z[1])
                t = {"split": [], "chunk": []}
                for _ in range(rounds):
                    t["split"].append(bench(split, n=16, reps=3))
                    t["chunk"].append(bench(chunk, n=16, reps=3))
                out.append(f"S={S}: {statistics.median(t['split']):7.1f} /"
                           f" {statistics.median(t['chunk']):7.1f}")
            diff = (z[0][0].int() - z[1][0].int()).abs().max().item()
            print(f"B={B:2d} pos={p:5d}  " + "  ".join(out)
                  + f"  max |dcode| {diff}")


def gqa_ab(kv_dtype="f16", page_size=0, positions=(512, 2048, 4096, 8192),
           batches=(1, 8, 32), rounds=5, gqa_splits=(4, 8, 16, 32)):
    """Decode-row attention alone in an isolated hipGraph at the 8B shape (32
    heads, kv_mul 4, hd 128, Q80 output): B rows of B distinct sequences, all
    at position p. k_attn_split + combine (attn_rows, or attn_paged with
    --page-size: pages mapped in a scrambled order) at the decode schedule's S
    against k_attn_gqa + combine on the same cache at the same S and at every
    S of gqa_splits, and with --kv-dtype q80 against the f16 k_attn_gqa on
    the dequantised values (unpaged), interleaved over `rounds`: median
    (min..max) us per call, the fraction of 6.3 TB/s that the distinct K/V
    bytes (codes and scales) reach at the schedule's S, and the largest |code|
    difference between the Q80 outputs of the first two there.

      python tools/kernel_bench.py gqa
      python tools/kernel_bench.py gqa --kv-dtype q80 [--page-size 64]"""
    H0, hd, kvd, kv_mul = 32, 128, 1024, 4
    P, q80 = page_size, kv_dtype == "q80"
    seq = max(positions) + 64
    assert seq % (P or 1) == 0, "a sequence is whole pages"
    print(f"\n-- decode-row attention, isolated graph, 8B shape, {kv_dtype} KV"
          f"{f', pages of {P}' if P else ''}, Q80 out "
          "(us per call: median (min..max)) --")
    for B in batches:
        n = B * seq
        if q80:
            flat = [torch.randint(-127, 128, (n, kvd), device=dev, generator=g)
                    .to(torch.int8) for _ in range(2)]
            flat += [(a / 127 * (0.5 + torch.rand(n, kvd // 32, device=dev,
                                                  generator=g))).half()
                     for a in (0.3, 1.0)]
            f16 = [(c.float() * s.float().repeat_interleave(32, dim=1)).half()
                   for c, s in zip(flat[:2], flat[2:])]
        else:
            flat = [(torch.randn(n, kvd, device=dev, generator=g) * 0.3).half(),
                    torch.randn(n, kvd, device=dev, generator=g).half()]
        planes, where, form = flat, (), "_rows"
        if P:  # pool row perm[j] * P + i holds flat row j * P + i
            perm = torch.randperm(n // P, device=dev, generator=g)
            src = (perm.argsort()[:, None] * P
                   + torch.arange(P, device=dev)).reshape(-1)
            planes = [t[src] for t in flat]
            where = (perm.to(torch.int32).reshape(B, -1).contiguous(), P)
            form = "_paged"
        kw = dict(zip(("k_scales", "v_scales"), planes[2:]))
        qv = torch.randn(B, H0 * hd, device=dev, generator=g)
        y = torch.zeros(B, H0 * hd, device=dev)
        z = [[torch.zeros(B, H0 * hd, dtype=torch.int8, device=dev),
              torch.zeros(B, H0 * hd // 32, device=dev),
              torch.zeros(B, H0 * hd // 32, device=dev)] for _ in range(2)]
        for p in positions:
            def i32(x):
                return torch.tensor(x, dtype=torch.int32, device=dev)
            rows = i32([[b * seq // (P or 1), p] for b in range(B)])
            flat_rows = i32([[b * seq, p] for b in range(B)])
            S0 = 8 if p < 512 else 16 if p < 2048 else 32
            cands = {}
            for name, S in [("split", S0), ("gqa", S0)] + [
                    (f"gqa S={S}", S) for S in gqa_splits if S != S0] + [
                    ("gqa f16", S0)] * q80:
                ml = torch.zeros(B * H0 * S * 2, device=dev)
                osc = torch.zeros(B * H0 * S * hd, device=dev)
                tail = (B, H0, kv_mul, hd, S, ml, osc, *z[name != "split"])
                if name == "gqa f16":
                    cands[name] = lambda tail=tail: k.attn_gqa_rows(
                        qv, H0 * hd, *f16, y, flat_rows, *tail)
                    continue
                fn = getattr(k, ("attn" if name == "split" else "attn_gqa")
                             + form)
                cands[name] = lambda fn=fn, tail=tail: fn(
                    qv, H0 * hd, *planes[:2], y, rows, *where, *tail, **kw)
            t = {name: [] for name in cands}
            for _ in range(rounds):
                for name, fn in cands.items():
                    t[name].append(bench(fn, n=16, reps=3))
            cands["split"](), cands["gqa"]()
            diff = (z[0][0].int() - z[1][0].int()).abs().max().item()
            # distinct K and V bytes: codes and scales, or halves
            nbytes = B * (p + 1) * kvd * 2 * (1 + 2 / 32 if q80 else 2)
            tbs = nbytes / statistics.median(t["gqa"]) / 1e6
            print(f"B={B:2d} pos={p:5d} S={S0:2d}  " + "  ".join(
                f"{name}: {statistics.median(v):6.1f} ({min(v):.1f}..{max(v):.1f})"
                for name, v in t.items())
                + f"  gqa {tbs:4.2f} TB/s ({100 * tbs / 6.3:2.0f}% of 6.3)"
                f"  max |dcode| {diff}", flush=True)
        del flat, planes
        f16 = None


def prefix_ab(kv_dtype="f16", page_size=64, batches=(2, 8, 32),
              prefixes=(256, 1024, 3584), suffixes=(64, 512), rounds=3,
              pre_splits=(4, 8, 16, 32)):
    """Decode-row attention of B sequences behind one shared prefix, alone in
    an isolated hipGraph at the 8B shape (32 heads, kv_mul 4, hd 128, Q80
    output, paged cache): every row has the same `prefix` leading tokens (the
    same pool pages, one group) and `suffix` tokens of its own. k_attn_split
    + combine (attn_paged) and k_attn_gqa + combine (attn_gqa_paged), which
    read the prefix once per row, against the three launches of
    attn_prefix_paged at every S_pre of pre_splits, all at the decode
    schedule's S, interleaved over `rounds`: median (min..max) us per call.

      python tools/kernel_bench.py prefix [--kv-dtype q80]"""
    H0, hd, kvd, kv_mul, P = 32, 128, 1024, 4, page_size
    q80 = kv_dtype == "q80"
    print(f"\n-- shared-prefix decode attention, isolated graph, 8B shape, "
          f"{kv_dtype} KV, pages of {P}, Q80 out "
          "(us per call: median (min..max)) --")

    def i32(x):
        return torch.tensor(x, dtype=torch.int32, device=dev)

    for B in batches:
        for N in prefixes:
            for sfx in suffixes:
                pos, n_pre = N + sfx, N // P
                own = sfx // P + 1
                pages = n_pre + B * own
                perm = torch.randperm(pages, generator=torch.Generator()
                                      .manual_seed(pages)).tolist()
                pt = i32([perm[:n_pre] + perm[n_pre + b * own:
                                              n_pre + (b + 1) * own]
                          for b in range(B)])
                n = pages * P
                if q80:
                    planes = [torch.randint(-127, 128, (n, kvd), device=dev,
                                            generator=g).to(torch.int8)
                              for _ in range(2)]
                    planes += [(a / 127 * (0.5 + torch.rand(
                        n, kvd // 32, device=dev, generator=g))).half()
                        for a in (0.3, 1.0)]
                else:
                    planes = [
                        (torch.randn(n, kvd, device=dev, generator=g) * 0.3).half(),
                        torch.randn(n, kvd, device=dev, generator=g).half()]
                kw = dict(zip(("k_scales", "v_scales"), planes[2:]))
                qv = torch.randn(B, H0 * hd, device=dev, generator=g)
                y = torch.zeros(B, H0 * hd, device=dev)
                z = [torch.zeros(B, H0 * hd, dtype=torch.int8, device=dev),
                     torch.zeros(B, H0 * hd // 32, device=dev),
                     torch.zeros(B, H0 * hd // 32, device=dev)]
                rows = i32([[b * pt.shape[1], pos] for b in range(B)])
                tables = (i32([[0, N]] * B), i32([[0, B]] + [[0, 0]] * 15),
                          i32(list(range(B))), i32([1]))
                S = 8 if pos < 512 else 16 if pos < 2048 else 32
                ml = torch.zeros(B * H0 * S * 2, device=dev)
                osc = torch.zeros(B * H0 * S * hd, device=dev)
                head = (qv, H0 * hd, *planes[:2], y, rows, pt, P)
                tail = (B, H0, kv_mul, hd, S, ml, osc)
                cands = {
                    "split": lambda: k.attn_paged(*head, *tail, *z, **kw),
                    "gqa": lambda: k.attn_gqa_paged(*head, *tail, *z, **kw)}
                for sp in pre_splits:
                    pre = (torch.zeros(B * H0 * sp * 2, device=dev),
                           torch.zeros(B * H0 * sp * hd, device=dev))
                    cands[f"prefix S_pre={sp}"] = lambda sp=sp, pre=pre: \
                        k.attn_prefix_paged(*head, *tables, *tail, sp, *pre,
                                            *z, **kw)
                t = {name: [] for name in cands}
                for _ in range(rounds):
                    for name, fn in cands.items():
                        t[name].append(bench(fn, n=16, reps=3))
                print(f"B={B:2d} prefix={N:4d} suffix={sfx:3d} S={S:2d}  "
                      + "  ".join(
                          f"{name}: {statistics.median(v):6.1f} "
                          f"({min(v):.1f}..{max(v):.1f})"
                          for name, v in t.items()), flush=True)
                del planes


def chunk_forms_ab(kv_dtype="f16", page_size=0, positions=(512, 2048, 4096, 8192),
                   batches=(32,), rounds=3):
    """The paged and Q80 forms of the chunk attention in an isolated hipGraph
    at the 8B shape (Q80 output), B rows of one sequence at first position p,
    at the S a row step of the decode schedule takes there (16 below 2048,
    else 32). Columns, interleaved over `rounds`, median us per call:

      parent      what such a step launches with the option off: attn_paged
                  with --page-size, else attn_rows (k_attn_split + combine)
      chunk       attn_chunk_paged / attn_chunk_rows on the same cache
      chunk flat  (--page-size) attn_chunk_rows on the same rows unpaged:
                  the difference to `chunk` is the cost of the page lookup
      chunk f16   (--kv-dtype q80) the same form on the dequantised values
                  as an f16 cache: what the halved loads bring

    Pages are mapped in a scrambled order.

      python tools/kernel_bench.py chunk --page-size 64
      python tools/kernel_bench.py chunk --kv-dtype q80 [--page-size 64]
      python tools/kernel_bench.py chunk-rows --kv-dtype q80     B = 4 .. 32"""
    H0, hd, kvd, kv_mul = 32, 128, 1024, 4
    P, q80 = page_size, kv_dtype == "q80"
    seq = (max(positions) + 64 + 255) // 256 * 256
    if q80:
        flat = [torch.randint(-127, 128, (seq, kvd), device=dev, generator=g)
                .to(torch.int8) for _ in range(2)]
        flat += [(a / 127 * (0.5 + torch.rand(seq, kvd // 32, device=dev,
                                              generator=g))).half()
                 for a in (0.3, 1.0)]
        f16 = [(c.float() * s.float().repeat_interleave(32, dim=1)).half()
               for c, s in zip(flat[:2], flat[2:])]
    else:
        flat = [(torch.randn(seq, kvd, device=dev, generator=g) * 0.3).half(),
                torch.randn(seq, kvd, device=dev, generator=g).half()]

    def i32(x):
        return torch.tensor(x, dtype=torch.int32, device=dev)

    def scales(planes):
        return dict(zip(("k_scales", "v_scales"), planes[2:]))

    if P:  # pool row perm[j] * P + i holds flat row j * P + i
        perm = torch.randperm(seq // P, device=dev, generator=g)
        src = (perm.argsort()[:, None] * P
               + torch.arange(P, device=dev)).reshape(-1)
        pool = [t[src] for t in flat]
        pt = perm.to(torch.int32).reshape(1, -1).contiguous()
    print(f"\n-- chunk attention forms, isolated graph, 8B shape, {kv_dtype} KV"
          f"{f', pages of {P}' if P else ''}, Q80 out (median us per call) --")
    for B in batches:
        qv = torch.randn(B, H0 * hd, device=dev, generator=g)
        y = torch.zeros(B, H0 * hd, device=dev)
        z = [torch.zeros(B, H0 * hd, dtype=torch.int8, device=dev),
             torch.zeros(B, H0 * hd // 32, device=dev),
             torch.zeros(B, H0 * hd // 32, device=dev)]
        runs = i32([[0, B]])
        for p in positions:
            S = 16 if p < 2048 else 32
            rows = i32([[0, p + b] for b in range(B)])
            ml = torch.zeros(B * H0 * S * 2, device=dev)
            osc = torch.zeros(B * H0 * S * hd, device=dev)
            tail = (B, H0, kv_mul, hd, S, ml, osc, *z)

            def rows_form(planes, chunk):
                if chunk:
                    return lambda: k.attn_chunk_rows(
                        qv, H0 * hd, *planes[:2], y, rows, runs, 1, *tail,
                        **scales(planes))
                return lambda: k.attn_rows(qv, H0 * hd, *planes[:2], y, rows,
                                           *tail, **scales(planes))

            def paged_form(chunk):
                if chunk:
                    return lambda: k.attn_chunk_paged(
                        qv, H0 * hd, *pool[:2], y, rows, pt, P, runs, 1, *tail,
                        **scales(pool))
                return lambda: k.attn_paged(qv, H0 * hd, *pool[:2], y, rows, pt,
                                            P, *tail, **scales(pool))

            form = paged_form if P else lambda c: rows_form(flat, c)
            cands = {"parent": form(False), "chunk": form(True)}
            if P:
                cands["chunk flat"] = rows_form(flat, True)
            if q80:
                cands["chunk f16"] = rows_form(f16, True)
            t = {name: [] for name in cands}
            for _ in range(rounds):
                for name, fn in cands.items():
                    t[name].append(bench(fn, n=16, reps=3))
            print(f"B={B:2d} pos={p:5d} S={S:2d}  " + "  ".join(
                f"{name}: {statistics.median(v):7.1f}" for name, v in t.items()))


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


def stream_ab(rounds=3, batches=(8, 16, 32), sweep=False):
    """q40_gemm_stream against the launches it replaces, alone in an isolated
    hipGraph at the 8B shapes, NB rows: `parent` is q40_gemm with its K-split
    reduce, plus add_ssq on the down-projections (wo, w2), where `stream` is
    q40_gemm_stream_resid. The graph rotates over weight copies that together
    exceed 300 MB (see resid_ab), the candidates are interleaved over
    `rounds`; median us per call and the stream's weight bytes/s against the
    6.3 TB/s ceiling. --sweep adds every (rows, waves) work split of the
    stream kernel, the measurement stream_shape()'s rule comes from.

      python tools/kernel_bench.py stream [--sweep]"""
    part = torch.zeros(32 * 32 * 8192, device=dev)
    print("\n-- q40_gemm_stream vs q40_gemm (+reduce, +add_ssq), isolated graph, "
          "rotating >300 MB of weights (median us per call) --")
    for tag, d, n, resid in (("wo", 4096, 4096, True), ("w2", 4096, 14336, True),
                             ("qkv", 6144, 4096, False), ("w13", 28672, 4096, False),
                             ("cls", 128256, 4096, False)):
        nbytes = d * n * 0.5625
        copies = int(300e6 // nbytes) + 1
        qs = torch.randint(0, 256, (copies, d, n // 2), dtype=torch.uint8,
                           device=dev, generator=g)
        sc = (torch.rand((copies, d, n // 32), device=dev, generator=g)
              * 0.01).to(torch.float16)
        xq, xs, xbs = mkx(32, n)
        y = torch.zeros(32, d, device=dev)
        xr = torch.zeros(32, d, device=dev)
        sq = torch.zeros(32, 16 * 32, device=dev)
        it = [0]

        def parent(B):
            i = it[0] % copies
            it[0] += 1
            k.q40_gemm(qs[i], sc[i], xq, xs, y, B, part)
            if resid:
                k.add_ssq(xr[:B], y[:B], sq, B)

        def stream(B, rows=0, waves=0):
            i = it[0] % copies
            it[0] += 1
            if resid:
                k.q40_gemm_stream_resid(qs[i], sc[i], xq, xs, xbs, xr, sq, B,
                                        rows, waves)
            else:
                k.q40_gemm_stream(qs[i], sc[i], xq, xs, xbs, y, B, rows, waves)

        for B in batches:
            cands = {"parent": lambda: parent(B), "stream": lambda: stream(B)}
            if sweep:
                for rows in (16, 32):
                    for waves in (4, 8):
                        cands[f"{rows}r{waves}w"] = (
                            lambda r=rows, w=waves: stream(B, r, w))
            t = {name: [] for name in cands}
            for _ in range(rounds):
                for name, fn in cands.items():
                    it[0] = 0
                    t[name].append(bench(fn, n=max(16, copies), reps=3))
            med = {name: statistics.median(v) for name, v in t.items()}
            print(f"{tag:4s} {d:6d}x{n:<5d} NB={B:2d}  " + "  ".join(
                f"{name}: {v:7.2f}" for name, v in med.items())
                + f"  stream {nbytes / med['stream'] / 1e6:5.2f} TB/s"
                f" ({100 * nbytes / med['stream'] / 6.3e6:3.0f}% of 6.3)")
        del qs, sc


def tile_ab(rounds=3, batches=(64, 96, 128)):
    """q40_gemm_tile at 64, 96 and 128 rows against the parent's best for the
    same rows: q40_gemm_stream once per 32 rows (its residual form on wo and
    w2, which is what replaces q40_gemm + add_ssq there). Weights rotate and
    candidates interleave as in stream_ab; median us per call and the tile
    kernel's weight bytes/s against the 6.3 TB/s ceiling.

      python tools/kernel_bench.py tile"""
    print("\n-- q40_gemm_tile vs ceil(rows / 32) x q40_gemm_stream, isolated "
          "graph, rotating >300 MB of weights (median us per call) --")
    for tag, d, n, resid in (("wo", 4096, 4096, True), ("w2", 4096, 14336, True),
                             ("qkv", 6144, 4096, False), ("w13", 28672, 4096, False),
                             ("cls", 128256, 4096, False)):
        nbytes = d * n * 0.5625
        copies = int(300e6 // nbytes) + 1
        qs = torch.randint(0, 256, (copies, d, n // 2), dtype=torch.uint8,
                           device=dev, generator=g)
        sc = (torch.rand((copies, d, n // 32), device=dev, generator=g)
              * 0.01).to(torch.float16)
        xq, xs, xbs = mkx(128, n)
        y = torch.zeros(128, d, device=dev)
        xr = torch.zeros(128, d, device=dev)
        sq = torch.zeros(128, 16 * 32, device=dev)
        it = [0]

        def stream(B):
            i = it[0] % copies
            it[0] += 1
            for b0 in range(0, B, 32):
                r = slice(b0, min(b0 + 32, B))
                acts = (xq[r], xs[r], xbs[r])
                if resid:
                    k.q40_gemm_stream_resid(qs[i], sc[i], *acts, xr[r], sq[r],
                                            r.stop - b0)
                else:
                    k.q40_gemm_stream(qs[i], sc[i], *acts, y[r], r.stop - b0)

        def tile(B):
            i = it[0] % copies
            it[0] += 1
            if resid:
                k.q40_gemm_tile_resid(qs[i], sc[i], xq, xs, xbs, xr, sq, B)
            else:
                k.q40_gemm_tile(qs[i], sc[i], xq, xs, xbs, y, B)

        for B in batches:
            cands = {"stream": lambda: stream(B), "tile": lambda: tile(B)}
            t = {name: [] for name in cands}
            for _ in range(rounds):
                for name, fn in cands.items():
                    it[0] = 0
                    t[name].append(bench(fn, n=max(16, copies), reps=3))
            med = {name: statistics.median(v) for name, v in t.items()}
            print(f"{tag:4s} {d:6d}x{n:<5d} NB={B:3d}  " + "  ".join(
                f"{name}: {v:7.2f}" for name, v in med.items())
                + f"  tile {nbytes / med['tile'] / 1e6:5.2f} TB/s"
                f" ({100 * nbytes / med['tile'] / 6.3e6:3.0f}% of 6.3)",
                flush=True)
        del qs, sc


if sys.argv[1:] == ["attn"]:
    attn_ab()
    sys.exit(0)
if sys.argv[1:2] == ["prefix"]:
    prefix_ab("q80" if sys.argv[2:] == ["--kv-dtype", "q80"] else "f16")
    sys.exit(0)
if sys.argv[1:2] in (["chunk"], ["chunk-rows"], ["gqa"]) and len(sys.argv) > 2:
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("mode")
    ap.add_argument("--kv-dtype", choices=("f16", "q80"), default="f16")
    ap.add_argument("--page-size", type=int, default=0)
    ap.add_argument("--batches", default="1,8,32", help="gqa only")
    ap.add_argument("--positions", default="512,2048,4096,8192",
                    help="gqa only")
    a = ap.parse_args()
    if a.mode == "gqa":
        gqa_ab(a.kv_dtype, a.page_size,
               tuple(int(p) for p in a.positions.split(",")),
               tuple(int(b) for b in a.batches.split(",")))
        sys.exit(0)
    rows = (dict(positions=(512, 4096), batches=(4, 8, 16, 32))
            if a.mode == "chunk-rows" else {})
    chunk_forms_ab(a.kv_dtype, a.page_size, **rows)
    sys.exit(0)
if sys.argv[1:] == ["chunk"]:
    chunk_ab()
    sys.exit(0)
if sys.argv[1:] == ["gqa"]:
    gqa_ab()
    sys.exit(0)
if sys.argv[1:] == ["chunk-rows"]:
    chunk_ab(positions=(512, 4096), batches=(4, 8, 16, 32), splits=(16, 32))
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

if sys.argv[1:2] == ["stream"]:
    stream_ab(sweep="--sweep" in sys.argv[2:])
    sys.exit(0)
if sys.argv[1:] == ["tile"]:
    tile_ab()
    sys.exit(0)

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
