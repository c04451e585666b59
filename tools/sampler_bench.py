#!/usr/bin/env python3
"""What sampling costs per decoded token: the on-device sampler inside the
captured decode graph against the host path (`Sampler.sample_torch` behind a
logits-only graph, i.e. DLLAMA_DEVICE_SAMPLER=0), and the sampler alone.

End to end: a synthetic preset model decodes `--tokens` tokens per window
through the engine's own two loops (`decode_sample` / `decode_one` +
`Sampler.sample`), temperature 0.8, top-p 0.9. Both graphs are captured on
the same model and the windows alternate device, host, device, ... in one
process, each between device synchronisations, after a warm-up window of
each; the median and the min..max spread over `--repeats` windows are
reported.

Random-init weights give nearly flat logits (every token passes the top-p
cutoff, which overflows the device sampler's candidate list and makes it
fall back). `--logit-std` rescales the classifier so the logits row has
that standard deviation, which puts the candidate count of a Gaussian row
where a trained model's is; the measured count is printed with every row.
`--logit-std 0` leaves the flat logits alone and so measures the fallback.

Sampler alone: one recorded logits row rescaled to about 100, about 2000
and (just under) the cap's worth of candidates; per call for the device
sampler (parameter copy, three kernels, 16-byte read-back), for the kernels
alone (back-to-back launches between events) and for sample_torch.

  python tools/sampler_bench.py [--models llama-3.1-8b qwen3-30b-a3b]
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

T, TOPP = 0.8, 0.9


def candidates(row: torch.Tensor, temperature=T, topp=TOPP) -> int:
    p = torch.softmax(row.double() / temperature, dim=-1)
    return int((p >= (1.0 - topp) / (row.numel() - 1)).sum())


def spread(xs):
    return {"median": round(statistics.median(xs), 2),
            "min": round(min(xs), 2), "max": round(max(xs), 2)}


def build(name, seq_len, logit_std):
    from dllama_amd import model_file as mf
    from dllama_amd.models.config import ModelConfig
    from dllama_amd.models.hip_model import HipTransformer
    header = mf.preset_header(name, seq_len=seq_len)
    cfg = ModelConfig.from_header(header)
    model = HipTransformer.synthetic(cfg, device="cuda:0")
    torch.manual_seed(1234)
    prompt = torch.randint(0, cfg.vocab_size, (32,))
    row = model.forward(prompt, torch.arange(32))[-1]
    if logit_std > 0:
        # f16 scale plane of the classifier: scaling it scales the logits
        # (in place: the captured prefill graph holds its address)
        model.wcls.scales.mul_(logit_std / float(row.std()))
    return model, prompt


def end_to_end(name, args, logit_std):
    from dllama_amd.engine import InferenceEngine
    from dllama_amd.tokenizer import Sampler
    model, prompt = build(name, args.seq_len, logit_std)
    model.forward(prompt, torch.arange(32))
    # two graphs over the same buffers: with and without the sampler,
    # taken out of the model's store and put back for each window
    DECODE, graphs = ("decode", False), {}
    for mode, on in (("device", True), ("host", False)):
        model.device_sampling = on
        model.capture_decode_graph()
        graphs[mode] = model.graphs.entries.pop(DECODE)
    sampler = Sampler(model.cfg.vocab_size, T, TOPP, 12345)
    eng = InferenceEngine(model, sampler=sampler)
    stats = {"cands": [], "fallbacks": 0, "steps": 0}

    def window(mode, n):
        model.graphs.entries[DECODE] = graphs[mode]
        model._graph_pos = None
        model.device_sampling = mode == "device"
        eng.reset(32)
        token = 7
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "device":
            for _ in range(n):
                token = eng.decode_sample(token, sampler)
        else:
            for _ in range(n):
                token = sampler.sample(eng.decode_one(token))
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    for mode in ("device", "host"):
        window(mode, args.warmup)
    # outside the timed windows: how many candidates these logits give and
    # how often the device sampler gives up
    eng.reset(32)
    model.graphs.entries[DECODE] = graphs["device"]
    model._graph_pos = None
    token = 7
    for i in range(20):
        t = torch.tensor([token])
        got = model.forward_sample(t, torch.tensor([32 + i]), 0.5, T, TOPP)
        stats["cands"].append(candidates(model.last_logits()))
        stats["fallbacks"] += got is None
        token = got if got is not None else int(model.last_logits().argmax())
    rates = {"device": [], "host": []}
    for _ in range(args.repeats):
        for mode in ("device", "host"):
            rates[mode].append(window(mode, args.tokens))
    res = {"model": name, "logit_std": logit_std, "tokens_per_window": args.tokens,
           "repeats": args.repeats,
           "candidates_median": int(statistics.median(stats["cands"])),
           "device_fallbacks_of_20": int(stats["fallbacks"]),
           "device_tok_s": spread(rates["device"]),
           "host_tok_s": spread(rates["host"])}
    res["device_over_host"] = round(res["device_tok_s"]["median"]
                                    / res["host_tok_s"]["median"], 4)
    us = lambda r: 1e6 / r  # noqa: E731
    res["sampling_us_saved_per_token"] = round(
        us(res["host_tok_s"]["median"]) - us(res["device_tok_s"]["median"]), 1)
    print(json.dumps({"end_to_end": res}), flush=True)
    row = model.last_logits().clone()
    del model, eng, graphs
    torch.cuda.empty_cache()
    return row


def alone(row, args):
    """The sampler by itself on one recorded row, its spread rescaled to hit
    a candidate count."""
    from dllama_amd.ops import hip_ops
    from dllama_amd.ops.sampler import DeviceSampler
    from dllama_amd.tokenizer import Sampler
    v = row.numel()
    cap = int(hip_ops().sampler_max_candidates())
    smp = DeviceSampler(v, row.device)
    host = Sampler(v, T, TOPP, 1)
    unit = (row - row.mean()) / row.std()
    # f64 counts here, f32 in the kernel: stay 1% under the cap
    for target in (100, 2000, cap - cap // 100):
        lo, hi = 0.5, 40.0  # candidates fall as the spread grows
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            n = candidates(unit * mid)
            if n > target:
                lo = mid
            else:
                hi = mid
        r = (unit * hi).contiguous()
        n = candidates(r)
        coins = [(i + 0.5) / args.calls for i in range(args.calls)]

        def timed(fn):
            out = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for c in coins:
                    fn(c)
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) / len(coins) * 1e6)
            return spread(out)

        for c in coins[:10]:  # warm up both
            assert smp.sample(r, c, T, TOPP) is not None
            host.sample_torch(r, c)
        dev = timed(lambda c: smp.sample(r, c, T, TOPP))
        tor = timed(lambda c: host.sample_torch(r, c))
        kern = []
        for _ in range(args.repeats):
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            for _ in coins:
                smp.launch(r)
            e1.record()
            torch.cuda.synchronize()
            kern.append(e0.elapsed_time(e1) * 1e3 / len(coins))
        print(json.dumps({"sampler_alone": {
            "vocab": v, "candidates": n, "calls": args.calls,
            "device_call_us": dev, "device_kernels_us": spread(kern),
            "sample_torch_us": tor}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="*",
                    default=["llama-3.1-8b", "qwen3-30b-a3b"])
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--logit-std", type=float, nargs="*", default=[4.0, 0.0])
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sampler_bench needs a GPU"
    for name in args.models:
        row = None
        for std in args.logit_std:
            r = end_to_end(name, args, std)
            row = r if row is None else row
        alone(row, args)


if __name__ == "__main__":
    main()
