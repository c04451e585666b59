#!/usr/bin/env python3
"""Aggregate decode tokens/s of B sequences stepped together.

Synthetic Llama-3.1-8B with one KV slot per sequence. For each B the slots
are prefilled with a short random prompt, then every step is one
`forward_rows_sample` call at temperature 0: the replay of the captured
B-row graph (step + per-row samplers + table advance), its small staging
copy and the read-back of the B tokens, which are fed back as the next
step's input. That is the serving loop of `BatchEngine`, host work
included. The last entry is the single-sequence path (`forward_sample`
over the deferred-quant decode graph) timed the same way, the figure the
B=1 row path is compared with.

--kv-pages M runs the same loop on a paged KV cache of M pages (--page-size
rows each): slot s takes pages s, s+B, s+2B, ... so that no sequence is
contiguous in the pool. The single-sequence entry is left out then (a paged
model steps rows only). --context N starts the timed decode at position N:
the prompt is still --prefill tokens, the cache rows between hold zeros, and
every step reads all N of them, so long contexts are timed without paying
B long prefills. --kv-dtype q80 runs either form on the Q80 KV cache.
--logprobs turns set_logprobs on: every step also computes the rows' token
log-probabilities (top 20) in the graph and copies them back with the tokens.

Warmup and timing follow bench.py: untimed warmup steps on the shapes of
the timed window, then a host clock around `--steps` steps ending in a
device synchronise. Prints one JSON line.

Usage: python tools/batch_decode_bench.py [--steps 200] [--warmup 20]
           [--batches 1,8,32] [--context 4000 --seq-len 8192]
           [--kv-pages 4096 --page-size 64]
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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--model", default="llama-3.1-8b")
    ap.add_argument("--seq-len", type=int, default=4096)
    ap.add_argument("--prefill", type=int, default=32,
                    help="prompt tokens per sequence before the timed decode")
    ap.add_argument("--batches", default="1,2,4,8,16,32")
    ap.add_argument("--context", type=int, default=0,
                    help="position of the first timed decode step (default: "
                         "--prefill); rows past the prompt hold zeros")
    ap.add_argument("--kv-pages", type=int, default=0,
                    help="page the KV cache: pool of this many pages")
    ap.add_argument("--page-size", type=int, default=64)
    ap.add_argument("--kv-dtype", default=None, choices=["f16", "f32", "q80"],
                    help="KV cache format (default: the model's, f16)")
    ap.add_argument("--logprobs", action="store_true",
                    help="set_logprobs(True): log-probabilities in every step")
    args = ap.parse_args()
    context = max(args.context, args.prefill)
    if not torch.cuda.is_available():
        sys.exit("error: batch_decode_bench needs a GPU")  # no CPU fall-back

    from bench import _use_built_extension
    from dllama_amd import model_file as mf
    from dllama_amd.models.config import ModelConfig
    from dllama_amd.models.hip_model import HipTransformer
    _use_built_extension()

    batches = [int(b) for b in args.batches.split(",")]
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    header = mf.preset_header(args.model, seq_len=args.seq_len)
    cfg = ModelConfig.from_header(header)
    t0 = time.time()
    paging = (dict(kv_pages=args.kv_pages, page_size=args.page_size)
              if args.kv_pages else {})
    if args.kv_dtype is not None:
        paging["kv_dtype"] = args.kv_dtype
    model =HipTransformer.synthetic(cfg, device=device, n_slots=max(batches),
                                     **paging)
    model.device_sampling = True
    model.set_logprobs(args.logprobs)
    torch.cuda.synchronize(device)
    print(f"# built synthetic {args.model} with {model.n_slots} KV slots in "
          f"{time.time() - t0:.1f}s", file=sys.stderr)
    last = context + args.warmup + args.steps
    if last > cfg.seq_len:
        sys.exit("error: context + warmup + steps exceed --seq-len")
    pages_per_slot = -(-last // args.page_size)
    if args.kv_pages and pages_per_slot * max(batches) > args.kv_pages:
        sys.exit(f"error: {max(batches)} sequences of {last} positions need "
                 f"{pages_per_slot * max(batches)} pages")

    torch.manual_seed(1234)
    prompt = torch.randint(0, cfg.vocab_size, (args.prefill,)).tolist()

    def timed(step):
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize(device)
        return time.perf_counter() - t0

    def entry(elapsed, B):
        return {"tokens_per_s": round(B * args.steps / elapsed, 2),
                "ms_per_step": round(elapsed / args.steps * 1000.0, 4)}

    rows = {}
    for B in batches:
        slots = list(range(B))
        if args.kv_pages:
            for s in range(model.n_slots):
                model.clear_slot(s)
            for s in slots:  # interleaved: no sequence is contiguous
                model.set_slot_pages(s, [i * B + s
                                         for i in range(pages_per_slot)])
        for s in slots:  # every sequence's prompt, one chunk per step
            for i in range(0, args.prefill, model.n_batches):
                chunk = prompt[i: i + model.n_batches]
                model.forward_rows(chunk, [s] * len(chunk),
                                   list(range(i, i + len(chunk))))
        state = {"tokens": [7] * B, "pos": context}
        zeros, topps = [0.0] * B, [0.9] * B

        def step():
            picked = model.forward_rows_sample(
                state["tokens"], slots, [state["pos"]] * B, zeros, zeros, topps)
            state["tokens"] = picked
            state["pos"] += 1

        elapsed = timed(step)
        assert model.graphs.get(("rows", B, model.logprobs)) is not None, \
            "the timed steps were not graph replays"
        rows[str(B)] = entry(elapsed, B)
        print(f"# B={B}: {rows[str(B)]}", file=sys.stderr)

    # the single-sequence path, same loop shape: forward_sample replays the
    # deferred-quant decode graph with the sampler inside
    single_entry = None
    if not args.kv_pages:
        model.forward(torch.tensor(prompt[: model.n_batches]),
                      torch.arange(min(args.prefill, model.n_batches)))
        model.capture_decode_graph()
        state = {"token": 7, "pos": context}

        def single():
            state["token"] = model.forward_sample(
                torch.tensor([state["token"]]), torch.tensor([state["pos"]]),
                0.0, 0.0, 0.9)
            state["pos"] += 1

        single_entry = entry(timed(single), 1)

    mname = "Llama-3.1-8B" if args.model == "llama-3.1-8b" else args.model
    print(json.dumps({
        "metric": f"aggregate decode tokens/s by batch ({mname} Q40, "
                  "forward_rows_sample graphs)",
        "unit": "tokens/s",
        "higher_is_better": True,
        "steps": args.steps,
        "warmup": args.warmup,
        "rows": rows,
        "single_stream_forward_sample": single_entry,
        "config": {"model": args.model, "seq_len": args.seq_len,
                   "prefill": args.prefill, "context": context,
                   "kv_pages": args.kv_pages,
                   "page_size": args.page_size if args.kv_pages else None,
                   "n_slots": model.n_slots,
                   "kv_dtype": model.kv_dtype,
                   "kv_cache_bytes": model.kv_cache_bytes(),
                   "sampling": "on device, temperature 0",
                   "logprobs": args.logprobs,
                   "data": "synthetic (random-init weights, random prompt)"},
    }))


if __name__ == "__main__":
    main()
