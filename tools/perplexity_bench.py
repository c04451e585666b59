#!/usr/bin/env python3
"""Tokens/s of the `dllama perplexity` loop, both ways of scoring a chunk.

Synthetic Llama-3.1-8B, a random prompt of --tokens tokens fed in chunks of
32 as `run_perplexity` feeds them. Per chunk either
  host    the [32, vocab] logits block is copied to the host and every row
          goes through logsumexp there (what `dllama perplexity` did), or
  device  `model.logprob_targets(logits, next_tokens)`: the logprob kernels
          at k = 0, 32 floats come back (what it does now on the HIP
          backend).
The two are timed alternately, --repeats times each, after one untimed pass
of either; a host clock around a pass that ends in a device synchronise.
Prints one JSON line with the best and the spread of each.

Usage: python tools/perplexity_bench.py [--tokens 2048] [--repeats 3]
"""

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--model", default="llama-3.1-8b")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("error: perplexity_bench needs a GPU")  # no CPU fall-back

    from bench import _use_built_extension
    from dllama_amd import model_file as mf
    from dllama_amd.models.config import ModelConfig
    from dllama_amd.models.hip_model import HipTransformer
    _use_built_extension()

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    header = mf.preset_header(args.model, seq_len=max(4096, args.tokens))
    cfg = ModelConfig.from_header(header)
    model = HipTransformer.synthetic(cfg, device=device)
    torch.manual_seed(1234)
    tokens = torch.randint(0, cfg.vocab_size, (args.tokens,)).tolist()
    nb = model.n_batches

    def one_pass(mode):
        nll, count = 0.0, 0
        for i in range(0, len(tokens) - 1, nb):
            chunk = tokens[i: i + nb]
            logits = model.forward(torch.tensor(chunk),
                                   torch.arange(i, i + len(chunk)))
            nxt = [tokens[i + j + 1] if i + j + 1 < len(tokens) else -1
                   for j in range(len(chunk))]
            if mode == "device":
                lps = model.logprob_targets(logits, nxt)
            else:
                host = logits.detach().float().cpu()
                lps = [float((host[j] - torch.logsumexp(host[j], dim=-1))[t])
                       if t >= 0 else 0.0 for j, t in enumerate(nxt)]
            for t, lp in zip(nxt, lps):
                if t >= 0:
                    nll -= lp
                    count += 1
        torch.cuda.synchronize(device)
        return nll / count

    def timed(mode):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        nll = one_pass(mode)
        return (len(tokens) - 1) / (time.perf_counter() - t0), nll

    for mode in ("host", "device"):
        one_pass(mode)  # untimed: captures the prefill graph, loads kernels
    rates = {"host": [], "device": []}
    nlls = {}
    for _ in range(args.repeats):
        for mode in ("host", "device"):
            rate, nlls[mode] = timed(mode)
            rates[mode].append(round(rate, 1))
    print(json.dumps({
        "metric": "perplexity loop tokens/s (32-token chunks)",
        "unit": "tokens/s", "higher_is_better": True,
        "tokens": args.tokens, "rates": rates,
        "best": {m: max(r) for m, r in rates.items()},
        "nll_per_token": nlls,
        "config": {"model": args.model,
                   "data": "synthetic (random-init weights, random prompt)"},
    }))


if __name__ == "__main__":
    main()
