#!/usr/bin/env python3
"""The MoE FFN of a multi-row step, parent launches against the
expert-grouped GEMM (DLLAMA_MOE_GEMM), on an MI355X.

  python tools/moe_gemm_bench.py ops   per-op, isolated hipGraphs, at the
      Qwen3-30B-A3B per-rank shapes (E = 128, top-8, W1|W3 (1536, 2048), W2
      (2048, 768)), NB in {2, 4, 8, 16, 32}, top-8 of random router logits:
        parent   q40_gemv_grouped + swiglu_q80 + q40_gemv_grouped
        grouped  moe_group + q40_gemm_grouped (SwiGLU) + q40_gemm_grouped
      A graph holds LAYERS calls, each on its own layer's weights (as a step
      walks the layers), so no call finds its experts cached by the one
      before. The candidates alternate over ROUNDS; median, min and max us
      per call, and the largest |y| difference between the two paths.
  python tools/moe_gemm_bench.py e2e [--layers N]   the synthetic
      qwen3-30b-a3b preset, option off and on in alternation on one model:
      prompt-chunk tok/s (32-row forward, captured graph) and ms per row
      step of 8 and 32 decode rows (forward_rows, captured graph).
"""

import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

E, KA, DIM, FF = 128, 8, 2048, 768
LAYERS, ROUNDS = 4, 5
dev = "cuda"


def graph_us(fn, reps=20):
    """us per call of fn() (itself LAYERS calls) from a captured graph."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        fn()
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        gr.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps / LAYERS * 1e6


def ops():
    from dllama_amd.ops import hip_ops
    from dllama_amd.ops import reference as R
    k = hip_ops()
    g = torch.Generator(device=dev).manual_seed(0)

    def planes(d, n):
        qs = torch.randint(0, 256, (E, d, n // 2), device=dev, generator=g,
                           dtype=torch.uint8)
        sc = (torch.rand(E, d, n // 32, device=dev, generator=g) * 0.01 + 0.001).half()
        return qs, sc

    w13 = [planes(2 * FF, DIM) for _ in range(LAYERS)]
    w2 = [planes(DIM, FF) for _ in range(LAYERS)]
    print(f"-- MoE FFN per layer, isolated graphs of {LAYERS} layers, "
          f"{ROUNDS} alternating rounds (us per layer: median [min .. max]) --")
    for NB in (2, 4, 8, 16, 32):
        S = NB * KA
        x = torch.randn(NB, DIM, device=dev, generator=g)
        xq = (torch.zeros(NB, DIM, dtype=torch.int8, device=dev),
              torch.zeros(NB, DIM // 32, device=dev),
              torch.zeros(NB, DIM // 32, device=dev))
        k.q80_quantize(x, *xq)
        logits = torch.randn(NB, E, generator=torch.Generator().manual_seed(NB))
        idx = R.moe_gate(logits, KA)[0].reshape(-1).to(torch.int32).to(dev)
        distinct = idx.unique().numel()
        out13 = torch.zeros(S, 2 * FF, device=dev)
        dq = [(torch.zeros(S, FF, dtype=torch.int8, device=dev),
               torch.zeros(S, FF // 32, device=dev),
               torch.zeros(S, FF // 32, device=dev)) for _ in range(2)]
        y = [torch.zeros(S, DIM, device=dev) for _ in range(2)]
        plan = torch.zeros(516 + 3 * 528, dtype=torch.int32, device=dev)

        def parent():
            for l in range(LAYERS):
                k.q40_gemv_grouped(*w13[l], *xq, idx, out13, KA)
                k.swiglu_q80(out13, out13[:, FF:], 2 * FF, FF, S, *dq[0])
                k.q40_gemv_grouped(*w2[l], *dq[0], idx, y[0], 1)

        def grouped():
            for l in range(LAYERS):
                k.moe_group(idx, plan, E)
                k.q40_gemm_grouped(*w13[l], xq[0], xq[1], plan, S, KA,
                                   oq=dq[1][0], os=dq[1][1], obs=dq[1][2])
                k.q40_gemm_grouped(*w2[l], dq[1][0], dq[1][1], plan, S, 1, y=y[1])

        t = {"parent": [], "grouped": []}
        for _ in range(ROUNDS):
            t["parent"].append(graph_us(parent))
            t["grouped"].append(graph_us(grouped))
        diff = (y[0] - y[1]).abs().max().item() / y[0].abs().max().item()
        med = {n: statistics.median(v) for n, v in t.items()}
        print(f"NB={NB:2d} S={S:3d} experts={distinct:3d}  " + "  ".join(
            f"{n}: {med[n]:7.1f} [{min(v):7.1f} .. {max(v):7.1f}]"
            for n, v in t.items())
            + f"  parent/grouped {med['parent'] / med['grouped']:.2f}"
            + f"  max |dy|/max|y| {diff:.2e}")


def e2e(layers):
    from bench import _use_built_extension
    from dllama_amd import model_file as mf
    from dllama_amd.models.config import ModelConfig
    from dllama_amd.models.hip_model import HipTransformer
    _use_built_extension()
    header = mf.preset_header("qwen3-30b-a3b", seq_len=1024)
    if layers:
        header.n_layers = layers
    cfg = ModelConfig.from_header(header)
    t0 = time.time()
    model = HipTransformer.synthetic(cfg, device=torch.device("cuda", 0), n_slots=32)
    torch.cuda.synchronize()
    print(f"-- synthetic qwen3-30b-a3b, {cfg.n_layers} layers, built in "
          f"{time.time() - t0:.0f}s; option off / on alternating, "
          f"{ROUNDS} rounds --")
    tokens = torch.randint(0, cfg.vocab_size, (32,),
                           generator=torch.Generator().manual_seed(1))

    def chunk():  # 8 full prompt chunks at positions 0..255
        for i in range(8):
            model.forward(tokens, torch.arange(32 * i, 32 * i + 32))

    def rows(B):
        def step():
            for p in range(8):
                model.forward_rows(tokens[:B].tolist(), list(range(B)), [300 + p] * B)
        return step

    cases = {"chunk 32 rows, tok/s": (chunk, lambda s: 256 / s),
             "row step B=8, ms": (rows(8), lambda s: s / 8 * 1e3),
             "row step B=32, ms": (rows(32), lambda s: s / 8 * 1e3)}
    res = {(n, on): [] for n in cases for on in (False, True)}
    for _ in range(ROUNDS):
        for on in (False, True):
            model.set_moe_gemm(on)
            for n, (fn, fig) in cases.items():
                fn()  # captures the step's graph
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                res[n, on].append(fig(time.perf_counter() - t0))
    for n in cases:
        print(f"{n:22s} " + "  ".join(
            f"{'on' if on else 'off'}: {statistics.median(res[n, on]):9.2f} "
            f"[{min(res[n, on]):9.2f} .. {max(res[n, on]):9.2f}]"
            for on in (False, True)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("section", choices=["ops", "e2e"])
    ap.add_argument("--layers", type=int, default=0,
                    help="e2e: layers of the preset to build (default: all 48)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("error: moe_gemm_bench needs a GPU")  # no CPU fall-back
    ops() if args.section == "ops" else e2e(args.layers)
