#!/usr/bin/env python3
"""Launch-trace pin for `HipTransformer`'s schedules.

Which kernels run, in what order and on which buffers is decided in Python
(`dllama_amd/models/hip_model.py`). This tool replays a matrix of model
configurations on the CPU with a recorder in place of the HIP extension
(`model.k`) and of the communicator (`model.comm`), and compares the
resulting `(kernel, args)` lists with two goldens. No GPU and no extension
build are needed: the kernels never run, only the launch sequence is
observed.

  tests/golden/launch_trace.json       the single-sequence step,
      `forward_buffers(B)`, over BATCHES x MODES;
  tests/golden/launch_trace_rows.json  row steps, `forward_rows`, over
      ADDRESSINGS (row table; row table + page table) x ROW_STEPS x
      ROW_MODES. A row step ignores `greedy_feedback` and `skip_logits`,
      and the modes pin that it does. The per-row sampler launches of
      `forward_rows_sample` are not traced: they are the same step followed
      by one sampler launch per row, which the GPU tests cover.

An argument is recorded in a canonical form that names no attribute:
scalars as they are (keyword names included), tensors as `(dtype, shape,
stride, storage_offset, storage_key)`. `storage_key` is a content digest
when the storage held non-zero data right after construction (weights,
norms, rope cache, embedding), else the ordinal of the storage's first
appearance in the trace (zero-initialised activation and scratch buffers,
temporaries). Renaming a buffer leaves a trace unchanged; another weight,
`ssq` slot, slice or argument order does not.

The first golden also holds a digest of every weight that
`HipTransformer.synthetic(cfg, device="cpu", seed=1234)` draws, keyed by
role and layer, so the RNG draw order stays comparable across commits.

  python tools/launch_trace.py            check against both goldens
  python tools/launch_trace.py --record   write both goldens
"""

import contextlib
import hashlib
import json
import os
import sys
import tempfile
from unittest import mock

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from dllama_amd import model_file as mf  # noqa: E402
from dllama_amd.models import hip_model as hm  # noqa: E402
from dllama_amd.models.config import ModelConfig  # noqa: E402
from dllama_amd.parallel.comm import SingleComm  # noqa: E402
from dllama_amd.quants import F32, Q80  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_trace.json")
GOLDEN_ROWS = os.path.join(ROOT, "tests", "golden", "launch_trace_rows.json")

# ------------------------------------------------------------------ matrix

_LLAMA = dict(arch_type=mf.ARCH_LLAMA, hidden_dim=128)
_QWEN3 = dict(arch_type=mf.ARCH_QWEN3, hidden_dim=96, norm_epsilon=1e-6)
_MOE = dict(arch_type=mf.ARCH_QWEN3_MOE, hidden_dim=96, norm_epsilon=1e-6,
            n_experts=4, n_active_experts=2, moe_hidden_dim=64)
# name -> (header fields, ModelConfig overrides). dim 256 where one size is
# enough: it also satisfies the TP deferred path's dim % 256 == 0
ARCHS = {
    "llama64": (dict(_LLAMA, dim=64), {}),
    "llama256": (dict(_LLAMA, dim=256), {}),
    "llama256_falcon": (dict(_LLAMA, dim=256, rope_type=mf.ROPE_FALCON), {}),
    "llama256_gelu": (dict(_LLAMA, dim=256, hidden_act=mf.HIDDEN_ACT_GELU), {}),
    "qwen3_64": (dict(_QWEN3, dim=64), {}),
    "qwen3_256": (dict(_QWEN3, dim=256), {}),
    # a .m header always gives qwen3 the falcon rope; only a hand-made
    # config reaches the separate q/k rmsnorm + rope_kv launches
    "qwen3_256_rope_llama": (dict(_QWEN3, dim=256),
                             dict(rope_type=mf.ROPE_LLAMA)),
    "qwen3moe64": (dict(_MOE, dim=64), {}),
    "qwen3moe256": (dict(_MOE, dim=256), {}),
}
# name -> (force_sync, sync_type)
SYNCS = {"plain": (False, Q80), "sync_q80": (True, Q80), "sync_f32": (True, F32)}
ENVS = {
    "none": {},
    "deferred0": {"DLLAMA_DEFERRED": "0"},
    "fused_ffn": {"DLLAMA_FUSED_FFN": "1"},
    "fused_moe": {"DLLAMA_FUSED_MOE": "1"},
    "ksplit2": {"DLLAMA_KSPLIT_RESID": "2"},
    "prefill_bf16": {"DLLAMA_PREFILL_BF16": "1"},
    "fused_sync0": {"DLLAMA_FUSED_SYNC": "0"},
    "splits4": {"DLLAMA_ATTN_SPLITS": "4"},
}
BATCHES = [1, 3, 8, 20, 32]
MODES = [(False, False), (True, False), (False, True)]  # (greedy, skip_logits)

# row steps. name -> (constructor arguments, {slot: pool pages}); no page is
# shared and every position of ROW_STEPS is mapped
ADDRESSINGS = {
    "table": (dict(n_slots=3), {}),
    "paged": (dict(n_slots=3, kv_pages=12, page_size=8),
              {0: [0, 1, 2], 1: [3, 4], 2: [5, 6, 7, 8]}),
}
# name -> (tokens, slots, positions)
ROW_STEPS = {
    # NB=1, a slot other than 0
    "one_decode_row": ([5], [1], [0]),
    # NB=4: the GEMV side of _mm
    "all_decode": ([7, 11, 13], [0, 1, 2], [3, 9, 20]),
    # two prompt chunks and one decode row, NB=16: the GEMM side of _mm
    "mixed": ([17, 19, 23, 29, 31, 37, 41, 43, 47],
              [0, 0, 0, 0, 0, 1, 2, 2, 2],
              [4, 5, 6, 7, 8, 10, 21, 22, 23]),
}
ROW_MODES = [(True, False), (False, True)]  # both ignored by a row step


def applies(arch: str, env: str) -> bool:
    """A flag that the arch can never reach is left out of the matrix."""
    moe = "moe" in arch
    if env == "fused_moe":
        return moe
    if env in ("fused_ffn", "prefill_bf16"):
        return not moe
    return True


def configs():
    for arch in ARCHS:
        for sync in SYNCS:
            for env in ENVS:
                if applies(arch, env):
                    yield arch, sync, env


# ---------------------------------------------------------------- recorder

def _sha(data: bytes, n: int) -> str:
    return hashlib.sha1(data).hexdigest()[:n]


def _storage_u8(t: torch.Tensor) -> torch.Tensor:
    return torch.tensor([], dtype=torch.uint8).set_(t.untyped_storage())


def tensor_digest(t: torch.Tensor) -> str:
    head = f"{t.dtype}{list(t.shape)}".encode()
    return _sha(head + t.contiguous().view(torch.uint8).numpy().tobytes(), 16)


def _walk_tensors(obj, seen, depth=0):
    """Every tensor reachable from obj through lists, dicts and attributes."""
    if isinstance(obj, torch.Tensor):
        yield obj
    elif id(obj) in seen or depth > 6:
        return
    elif isinstance(obj, (list, tuple)):
        seen.add(id(obj))
        for v in obj:
            yield from _walk_tensors(v, seen, depth + 1)
    elif isinstance(obj, dict):
        seen.add(id(obj))
        for v in obj.values():
            yield from _walk_tensors(v, seen, depth + 1)
    elif type(obj).__module__ == hm.__name__:
        seen.add(id(obj))
        yield from _walk_tensors(vars(obj), seen, depth + 1)


def content_keys(model) -> dict:
    """storage data_ptr -> content digest, for storages that are non-zero
    right after construction."""
    keys = {}
    for t in _walk_tensors(model, set()):
        ptr = t.untyped_storage().data_ptr()
        if ptr not in keys:
            raw = _storage_u8(t)
            keys[ptr] = (_sha(raw.numpy().tobytes(), 16) if raw.any()
                         else None)
    return {p: d for p, d in keys.items() if d is not None}


class Trace:
    """One ordered list of canonical (name, args, kwargs) calls."""

    def __init__(self, content: dict):
        self.content = content
        self.calls = []
        self.ordinals = {}
        self.keep = []  # keeps temporaries alive so data_ptrs stay unique

    def canon(self, a):
        if isinstance(a, torch.Tensor):
            self.keep.append(a)
            ptr = a.untyped_storage().data_ptr()
            key = self.content.get(ptr)
            if key is None:
                key = self.ordinals.setdefault(ptr, len(self.ordinals))
            return ["T", str(a.dtype), list(a.shape), list(a.stride()),
                    a.storage_offset(), key]
        if isinstance(a, (list, tuple)):
            return [self.canon(v) for v in a]
        if a is None or isinstance(a, (bool, int, float, str)):
            return a
        raise TypeError(f"unrecordable argument {type(a)}")

    def add(self, name, args, kwargs):
        self.calls.append([name, [self.canon(a) for a in args],
                           {k: self.canon(kwargs[k]) for k in sorted(kwargs)}])

    def lines(self):
        return [f"{c[0]}:{_sha(json.dumps(c).encode(), 12)}" for c in self.calls]


class RecordingKernels:
    """Stands in for the HIP extension: records every launch, runs nothing."""

    def __init__(self):
        self.trace = None

    def __getattr__(self, name):
        def launch(*args, **kwargs):
            self.trace.add(name, args, kwargs)
        return launch


class RecordingComm(SingleComm):
    def __init__(self, kernels: RecordingKernels):
        self.kernels = kernels

    def all_gather(self, out, x):
        self.kernels.trace.add("comm.all_gather", (out, x), {})
        return super().all_gather(out, x)

    def allreduce_(self, x):
        self.kernels.trace.add("comm.allreduce_", (x,), {})
        return super().allreduce_(x)


@contextlib.contextmanager
def _options(extra: dict):
    """The DLLAMA_* options in the environment replaced by `extra`."""
    saved = {k: v for k, v in os.environ.items() if k.startswith("DLLAMA_")}
    for k in saved:
        del os.environ[k]
    os.environ.update(extra)
    try:
        yield
    finally:
        for k in extra:
            del os.environ[k]
        os.environ.update(saved)


@contextlib.contextmanager
def _single_thread():
    """No kernel runs here, so torch's CPU work is thousands of tiny ops
    (`zero_`, copies, slices). With one thread they run inline; a wide
    intra-op pool left behind by an earlier caller in the same process
    would pay a fork-join for each of them."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def write_models(workdir: str) -> dict:
    paths = {}
    for arch, (fields, _) in ARCHS.items():
        h = mf.LlmHeader(n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64,
                         vocab_size=256, seq_len=64, rope_theta=10000,
                         **fields)
        h.finalize()
        paths[arch] = os.path.join(workdir, arch + ".m")
        mf.write_synthetic_model(paths[arch], h, seed=11)
    return paths


def _recorded_model(path: str, arch: str, sync: str, env: str, **ctor):
    """(model, its recording kernels, its content keys)."""
    force_sync, sync_type = SYNCS[sync]
    m = mf.ModelFile(path, sync_type=sync_type)
    cfg = ModelConfig.from_header(m.header)
    for k, v in ARCHS[arch][1].items():
        setattr(cfg, k, v)
    kernels = RecordingKernels()
    with _options(ENVS[env]), \
            mock.patch.object(hm, "hip_ops", lambda: kernels):
        model = hm.HipTransformer.from_file(
            m, cfg, device="cpu", comm=RecordingComm(kernels),
            force_sync=force_sync, **ctor)
    assert model.k is kernels and model.comm.kernels is kernels
    return model, kernels, content_keys(model)


def trace_config(path: str, arch: str, sync: str, env: str) -> list:
    """The traces of one model over BATCHES x MODES, each as a list of
    `(lines, calls)`."""
    model, kernels, content = _recorded_model(path, arch, sync, env)
    out = []
    for B in BATCHES:
        for greedy, skip in MODES:
            model.greedy_feedback, model.skip_logits = greedy, skip
            kernels.trace = Trace(content)
            model.forward_buffers(B)
            out.append((kernels.trace.lines(), kernels.trace.calls))
    return out


def trace_rows_config(path: str, arch: str, sync: str, env: str,
                      addressing: str) -> list:
    """The traces of one model over ROW_STEPS x ROW_MODES, through the
    public row API only."""
    ctor, pages = ADDRESSINGS[addressing]
    model, kernels, content = _recorded_model(path, arch, sync, env, **ctor)
    for slot, ids in pages.items():
        model.set_slot_pages(slot, ids)
    out = []
    for tokens, slots, positions in ROW_STEPS.values():
        for greedy, skip in ROW_MODES:
            model.greedy_feedback, model.skip_logits = greedy, skip
            kernels.trace = Trace(content)
            model.forward_rows(tokens, slots, positions)
            out.append((kernels.trace.lines(), kernels.trace.calls))
    return out


def synthetic_weights() -> dict:
    """Digest of every weight `synthetic` draws, keyed by role and layer."""
    out = {}
    for arch in ("llama64", "qwen3moe64"):
        h = mf.LlmHeader(n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64,
                         vocab_size=256, seq_len=64, rope_theta=10000,
                         **ARCHS[arch][0])
        cfg = ModelConfig.from_header(h.finalize())
        with _options({}), \
                mock.patch.object(hm, "hip_ops", RecordingKernels):
            model = hm.HipTransformer.synthetic(cfg, device="cpu", seed=1234)
        roles = {"embedding": model.embedding, "final_norm": model.final_norm,
                 "wcls": model.wcls}
        for l, lw in enumerate(model.layers):
            roles.update({f"layer{l}.{k}": v for k, v in lw.items()})
        digests = {}
        for role, w in roles.items():
            if isinstance(w, torch.Tensor):
                digests[role] = tensor_digest(w)
            else:
                digests[role + ".qs"] = tensor_digest(w.qs)
                digests[role + ".scales"] = tensor_digest(w.scales)
        out[arch] = dict(sorted(digests.items()))
    return out


# ------------------------------------------------------------ golden file

class Pin:
    """One golden file: its header (the axes of a model's runs), the models
    it covers, how a model is traced and how a run is labelled."""

    def __init__(self, path, header, models, trace, labels, weights=False):
        self.path = path
        self.header = json.loads(json.dumps(header))  # as the file holds it
        self.models = models    # () -> (name, arguments of trace after path)
        self.trace = trace
        self.labels = labels    # header -> one label per run of a model
        self.weights = weights  # also pins synthetic()'s draws


def _forward_models():
    for arch, sync, env in configs():
        yield f"{arch}/{sync}/{env}", (arch, sync, env)


def _rows_models():
    for arch, sync, env in configs():
        for addressing in ADDRESSINGS:
            yield (f"{arch}/{sync}/{env}/{addressing}",
                   (arch, sync, env, addressing))


def _mode_labels(head: str, modes) -> list:
    return [f"{head} greedy_feedback={g} skip_logits={s}" for g, s in modes]


FORWARD = Pin(
    GOLDEN, {"batches": BATCHES, "modes": MODES}, _forward_models,
    trace_config,
    lambda h: [s for B in h["batches"]
               for s in _mode_labels(f"B={B}", h["modes"])],
    weights=True)
ROWS = Pin(
    GOLDEN_ROWS,
    {"addressings": {a: {"constructor": ctor,
                         "pages": {str(s): p for s, p in pages.items()}}
                     for a, (ctor, pages) in ADDRESSINGS.items()},
     "steps": ROW_STEPS, "modes": ROW_MODES},
    _rows_models, trace_rows_config,
    lambda h: [s for step in h["steps"]
               for s in _mode_labels(f"step={step}", h["modes"])])
PINS = (FORWARD, ROWS)
_BODY = ("calls", "traces", "configs", "synthetic_weights")


def build_live(pin: Pin = FORWARD):
    """(golden-shaped dict, {config: [calls per trace]}) of this tree."""
    call_ids, traces, trace_ids = {}, [], {}
    cfgs, live_calls = {}, {}
    with _single_thread(), tempfile.TemporaryDirectory() as workdir:
        paths = write_models(workdir)
        for name, args in pin.models():
            ids = []
            results = pin.trace(paths[args[0]], *args)
            for lines, _ in results:
                t = tuple(call_ids.setdefault(s, len(call_ids)) for s in lines)
                if t not in trace_ids:
                    trace_ids[t] = len(traces)
                    traces.append(list(t))
                ids.append(trace_ids[t])
            cfgs[name] = ids
            live_calls[name] = [calls for _, calls in results]
        weights = synthetic_weights() if pin.weights else None
    gold = dict(pin.header)
    # "kernel:digest" of every distinct call; a trace lists indices into
    # it, a config lists one trace index per run, first header axis major
    gold.update(calls=list(call_ids), traces=traces, configs=cfgs)
    if pin.weights:
        gold["synthetic_weights"] = weights
    return gold, live_calls


def compare(gold: dict, live: dict, live_calls: dict,
            pin: Pin = FORWARD) -> list:
    """Human-readable mismatches (empty when the pin holds)."""
    errs = []
    for key in pin.header:
        if gold.get(key) != live[key]:
            errs.append(f"{key}: golden {gold.get(key)} != live {live[key]}")
    if sorted(gold["configs"]) != sorted(live["configs"]):
        errs.append("configuration matrix differs from the golden: "
                    f"{sorted(set(gold['configs']) ^ set(live['configs']))}")
    if errs:
        return errs
    labels = pin.labels(gold)
    for name, want_ids in gold["configs"].items():
        if len(want_ids) != len(live["configs"][name]):
            errs.append(f"{name}: golden {len(want_ids)} runs != live "
                        f"{len(live['configs'][name])}")
        for i, (wi, gi) in enumerate(zip(want_ids, live["configs"][name])):
            want = [gold["calls"][c] for c in gold["traces"][wi]]
            got = [live["calls"][c] for c in live["traces"][gi]]
            if want == got:
                continue
            at = next((j for j, (a, b) in enumerate(zip(want, got)) if a != b),
                      min(len(want), len(got)))
            calls = live_calls[name][i]
            errs.append(
                f"{name} {labels[i]}: "
                f"first difference at call {at} "
                f"(golden {len(want)} calls, live {len(got)})\n"
                f"  golden: {want[at] if at < len(want) else '<end>'}\n"
                f"  live:   {got[at] if at < len(got) else '<end>'}\n"
                f"  live call: {calls[at] if at < len(calls) else '<end>'}")
    for arch, want in gold.get("synthetic_weights", {}).items():
        got = live["synthetic_weights"].get(arch, {})
        for role in sorted(set(want) | set(got)):
            if want.get(role) != got.get(role):
                errs.append(f"synthetic {arch} {role}: golden "
                            f"{want.get(role)} != live {got.get(role)}")
    return errs


def dump(gold: dict) -> str:
    """One line per top-level list entry: compact and diffable."""
    def block(items, open_, close):
        return open_ + "\n" + ",\n".join(items) + "\n" + close
    js = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    parts = [f'"{k}":{js(v)}' for k, v in gold.items() if k not in _BODY]
    parts += [
        '"calls":' + block([js(c) for c in gold["calls"]], "[", "]"),
        '"traces":' + block([js(t) for t in gold["traces"]], "[", "]"),
        '"configs":' + block([f"{js(k)}:{js(v)}"
                              for k, v in gold["configs"].items()], "{", "}"),
    ]
    if "synthetic_weights" in gold:
        parts.append('"synthetic_weights":'
                     + json.dumps(gold["synthetic_weights"], indent=1))
    return "{\n" + ",\n".join(parts) + "\n}\n"


def main(argv):
    status = 0
    for pin in PINS:
        live, live_calls = build_live(pin)
        what = (f"{os.path.basename(pin.path)}: {len(live['configs'])} "
                f"models x {len(pin.labels(pin.header))} runs")
        if "--record" in argv:
            with open(pin.path, "w") as f:
                f.write(dump(live))
            print(f"recorded {what}, {len(live['traces'])} distinct traces, "
                  f"{len(live['calls'])} distinct calls")
            continue
        with open(pin.path) as f:
            gold = json.load(f)
        errs = compare(gold, live, live_calls, pin)
        for e in errs[:10]:
            print(e)
        print(f"{what}: {len(errs)} mismatches" if errs else
              f"launch traces match the golden ({what})")
        status |= bool(errs)
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
