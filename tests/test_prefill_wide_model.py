"""HipTransformer(prefill_rows=...).forward_prefill: prompt chunks of 33..128
rows against the CPU model, with the models, comparison and tolerance of
test_rows_model; decode steps after the chunk (a wrong K/V row anywhere in it
shows there); graph replays against eager chunks; where InferenceEngine cuts a
prompt; the refusals."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd.engine import InferenceEngine
from dllama_amd.models.cpu_model import CpuTransformer
from test_rows_model import TOL, _hip, _rel_err, models  # noqa: F401


def _tokens(n=128):
    return torch.randint(0, 256, (n,), generator=torch.Generator().manual_seed(6))


def _cpu(models, arch, n, decode=0, **kw):  # noqa: F811
    """CPU logits of the n-token prompt's last row, then `decode` greedy
    steps: [(token fed, logits)]."""
    m, cfg = models[arch]
    cpu, t = CpuTransformer(m, cfg, **kw), _tokens()
    for i in range(0, n, 32):
        rows = min(32, n - i)
        last = cpu.forward(t[i:i + rows], torch.arange(i, i + rows))[-1]
    steps, logits = [], last
    for p in range(n, n + decode):
        tok = int(logits.argmax())
        logits = cpu.forward(torch.tensor([tok]), torch.tensor([p]))[0]
        steps.append((tok, logits))
    return last, steps


# (arch, kv_dtype, prefill_rows, prompt rows, decode steps): a full llama
# chunk that fills seq_len 128; full chunks of 96 and (qwen3, seq_len 64) a
# partial one of 60, each followed by decode steps; a partial chunk on a Q80
# cache
CASES = [("llama", None, 128, 128, 0), ("llama", None, 96, 96, 4),
         ("llama", "q80", 128, 96, 4), ("qwen3", None, 64, 60, 4)]


@pytest.mark.parametrize("arch,kv_dtype,rows,n,decode", CASES)
def test_prefill_then_decode(models, arch, kv_dtype, rows, n, decode):  # noqa: F811
    kw = {"kv_dtype": kv_dtype} if kv_dtype else {}
    last, steps = _cpu(models, arch, n, decode, **kw)
    model = _hip(models, arch, prefill_rows=rows, **kw)
    got = model.forward_prefill(_tokens()[:n], torch.arange(n)).cpu()
    assert got.shape == (1, last.shape[0])
    assert _rel_err(got[0], last) < TOL[arch], (arch, "prompt")
    for i, (tok, want) in enumerate(steps):
        got = model.forward(torch.tensor([tok]), torch.tensor([n + i])).cpu()
        assert _rel_err(got[0], want) < TOL[arch], (arch, "decode", i)


def test_partial_chunks_mid_sequence(models):  # noqa: F811
    """45 rows at position 0, then 40 rows at 45: the second chunk's runs
    start mid-sequence and its last run is partial."""
    model, t = _hip(models, "llama", prefill_rows=128), _tokens()
    for p0, rows in ((0, 45), (45, 40)):
        got = model.forward_prefill(t[p0:p0 + rows],
                                    torch.arange(p0, p0 + rows)).cpu()
        err = _rel_err(got[0], _cpu(models, "llama", p0 + rows)[0])
        assert err < TOL["llama"], (p0, rows, err)


def test_graph_equals_eager(models):  # noqa: F811
    """Two replays of the captured full chunk, same bits as eager chunks. (At
    dim 64 the residual fold's 4 workgroups each own an ssq slot, so the float
    atomics have no order to differ in.)"""
    eager = _hip(models, "llama", prefill_rows=64)
    eager.graphs.failed.add("prefill_wide")
    graphed, t = _hip(models, "llama", prefill_rows=64), _tokens()
    for p0 in (0, 64):
        step = (t[p0:p0 + 64], torch.arange(p0, p0 + 64))
        a = eager.forward_prefill(*step).cpu().clone()
        b = graphed.forward_prefill(*step).cpu().clone()
        assert torch.equal(a, b), p0
    assert not eager.graphs.entries
    assert list(graphed.graphs.entries) == [("prefill_wide", False)]


@pytest.mark.parametrize("n,want", [(100, [("wide", 64), ("wide", 36)]),
                                    (70, [("wide", 64), ("narrow", 6)])])
def test_engine_cut(models, n, want):  # noqa: F811
    model, calls = _hip(models, "llama", prefill_rows=64), []
    wide, narrow = model.forward_prefill, model.forward
    model.forward_prefill = lambda t, p: (calls.append(("wide", len(t))),
                                          wide(t, p))[1]
    model.forward = lambda t, p: (calls.append(("narrow", len(t))),
                                  narrow(t, p))[1]
    engine = InferenceEngine(model)
    logits = engine.prefill(_tokens()[:n].tolist()).cpu()
    assert calls == want and engine.pos == n
    assert _rel_err(logits, _cpu(models, "llama", n)[0]) < TOL["llama"]


def test_refusals(models):  # noqa: F811
    with pytest.raises(ValueError, match="prefill_rows"):
        _hip(models, "llama", prefill_rows=48)
    with pytest.raises(ValueError, match="MoE"):
        _hip(models, "qwen3moe", prefill_rows=64)
    model = _hip(models, "llama", prefill_rows=128)
    for rows in (32, 129):
        with pytest.raises(ValueError, match="rows"):
            model.forward_prefill(torch.zeros(rows, dtype=torch.int64),
                                  torch.arange(rows))
    assert _hip(models, "llama").wide is None
