"""Prefill throughput probe: prompts of 512, 2k and 8k tokens through the
int8-MFMA GEMM path of a synthetic Llama-3.1-8B, in 32-token chunks, with the
chunk attention (set_chunk_attn) off and on, alternating. Per length and
setting: ms and tok/s of every repetition (each pays its own prefill-graph
captures, which the switch drops: the same cost in both settings), and the
tok/s of the last 512 tokens alone, where the context is longest.

  python tools/prefill_probe.py [lengths...]      default 512 2048 8192
    --ab stream                alternate set_stream_gemm instead (chunk attention
                               stays off): the weight-streaming GEMM
    --ab tile                  wide prefill (docs/DESIGN.md §14): the parent's best
                               (stream GEMM on, 32-row chunks) against models
                               built with prefill_rows 64 and 128, alternating,
                               then 32 graph-replayed B = 1 decode steps each
    --kv-dtype q80             a Q80 KV cache; "on" is set_chunk_attn(True, q80=True)
    --kv-pages M --page-size P a paged cache: the prompt goes through
                               forward_rows into slot 0, whose pages are mapped
                               in a scrambled order (M * P >= the longest prompt)"""
import argparse, os, sys, time, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from dllama_amd.model_file import preset_header
from dllama_amd.models.config import ModelConfig
from dllama_amd.models.hip_model import HipTransformer

ap = argparse.ArgumentParser()
ap.add_argument("lengths", type=int, nargs="*", default=[512, 2048, 8192])
ap.add_argument("--ab", choices=("chunk", "stream", "tile"), default="chunk")
ap.add_argument("--kv-dtype", choices=("f16", "q80"), default="f16")
ap.add_argument("--kv-pages", type=int, default=0)
ap.add_argument("--page-size", type=int, default=64)
a = ap.parse_args()
lengths, q80 = a.lengths, a.kv_dtype == "q80"
# --ab tile decodes at 512..543 after its prefills
h = preset_header("llama-3.1-8b",
                  seq_len=max(lengths + [544] if a.ab == "tile" else lengths))
cfg = ModelConfig.from_header(h)
m = HipTransformer.synthetic(cfg, kv_dtype=a.kv_dtype, kv_pages=a.kv_pages,
                             page_size=a.page_size)
prompt = torch.randint(0, 128256, (h.seq_len,))
if a.kv_pages:
    need = -(-max(lengths) // a.page_size)
    m.set_slot_pages(0, torch.randperm(a.kv_pages)[:need].tolist())


def step(i):
    if a.kv_pages:
        m.forward_rows(prompt[i:i+32].tolist(), [0] * 32, list(range(i, i+32)))
    else:
        m.forward(prompt[i:i+32], torch.arange(i, i+32))


def prefill(n):
    """(seconds for n tokens, seconds for the last 512 of them)."""
    if not a.kv_pages:
        m.pos.fill_(0)
    torch.cuda.synchronize(); t0 = t_tail = time.perf_counter()
    for i in range(0, n, 32):
        if i == n - 512:
            torch.cuda.synchronize(); t_tail = time.perf_counter()
        m.skip_logits = i < n - 32
        step(i)
        m.skip_logits = False
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return t1 - t0, t1 - t_tail


def tile_ab():
    """The stream-GEMM model in 32-row chunks against wide-prefill models."""
    m.set_stream_gemm(True)
    wide = {r: HipTransformer.synthetic(cfg, kv_dtype=a.kv_dtype, prefill_rows=r)
            for r in (64, 128)}
    runs = [("stream gemm, 32-row chunks", m, 0)] + [
        (f"prefill_rows {r}", w, r) for r, w in wide.items()]

    def go(model, rows, n):
        """n tokens, cut as InferenceEngine.prefill cuts them: wide chunks
        while more than 32 tokens remain, the rest through forward."""
        torch.cuda.synchronize(); t0 = time.perf_counter()
        i = 0
        while i < n:
            step, b = model.forward, min(32, n - i)
            if rows and n - i > 32:
                step, b = model.forward_prefill, min(rows, n - i)
            model.skip_logits = i + b < n
            step(prompt[i:i + b], torch.arange(i, i + b))
            model.skip_logits = False
            i += b
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for n in lengths:
        for rep in range(4):  # the first pays the graph captures
            for what, model, rows in runs:
                dt = go(model, rows, n)
                print(f"prefill {n:5d} tokens, {what}: {dt*1000:8.1f} ms = "
                      f"{n/dt:6.0f} tok/s{' (warm-up)' if rep == 0 else ''}",
                      flush=True)
    for what, model, _ in runs:
        model.capture_decode_graph()
    for rep in range(3):
        for what, model, _ in runs:
            go(model, 0, 512)
            tok = torch.tensor([1])
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for p in range(512, 544):
                model.forward(tok, torch.tensor([p]))
            torch.cuda.synchronize()
            print(f"decode at 512..543, {what}: "
                  f"{(time.perf_counter() - t0) / 32 * 1000:.3f} ms/token",
                  flush=True)


if a.ab == "tile":
    tile_ab()
    sys.exit(0)

for n in lengths:
    for rep in range(3):
        for on in (False, True):
            if a.ab == "stream":
                m.set_stream_gemm(on)
            else:
                m.set_chunk_attn(on, q80=q80)
            dt, tail = prefill(n)
            what = "stream gemm" if a.ab == "stream" else "chunk attn"
            print(f"prefill {n:5d} tokens, {what} {'on ' if on else 'off'}: "
                  f"{dt*1000:8.1f} ms = {n/dt:6.0f} tok/s; last 512: "
                  f"{512/tail:6.0f} tok/s", flush=True)
