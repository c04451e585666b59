"""HipTransformer(kv_dtype="q80"): the Q80 KV cache through the
single-sequence paths and the row steps of tests/test_rows_model.py (its
tiny models, tokens, schedule and tolerances), against the CPU oracle that
applies the same round trip, CpuTransformer(kv_dtype="q80")."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd import model_file as mf
from dllama_amd.models.config import ModelConfig
from dllama_amd.models.cpu_model import CpuTransformer
from dllama_amd.utils.testing import make_tiny_llama, make_tiny_qwen3

from test_rows_model import SCHEDULE, TOKENS, TOL, _drive, _rel_err

P = 4
# slot -> pool pages, scrambled and not monotonic (slots as SLOT_OF: the
# 9-, 5- and 13-token sequences live in slots 2, 0 and 3)
PAGES_OF = {2: [11, 3, 7], 0: [5, 14], 3: [2, 9, 0, 13]}
KV_PAGES = 16
N_PREFILL = 9  # the single sequence: TOKENS[arch][2], 9 + 4 tokens


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("kvq80")
    out = {}
    for arch in TOKENS:
        p = str(d / f"{arch}.m")
        if arch == "llama":
            make_tiny_llama(p, vocab_size=256)
        else:
            make_tiny_qwen3(p, moe=arch == "qwen3moe")
        m = mf.ModelFile(p)
        out[arch] = (m, ModelConfig.from_header(m.header))
    return out


@pytest.fixture(scope="module")
def oracle(models):
    """Per arch: the Q80-cache CPU logits of every sequence run alone, with
    the top-1/top-2 gap of every row above twice the tolerance. Computed
    once, shared, never written."""
    out = {}
    for arch, (m, cfg) in models.items():
        rows = []
        for toks in TOKENS[arch]:
            want = CpuTransformer(m, cfg, kv_dtype="q80").forward(
                torch.tensor(toks), torch.arange(len(toks)))
            top = torch.topk(want, 2).values
            gap = (top[:, 0] - top[:, 1]) / want.abs().max(dim=1).values
            assert gap.min().item() > 2 * TOL[arch], (arch, gap)
            rows.append(want)
        out[arch] = rows
    return out


def _hip(models, arch, **kw):
    from dllama_amd.models.hip_model import HipTransformer
    m, cfg = models[arch]
    hip = HipTransformer.from_file(m, cfg, kv_dtype="q80", **kw)
    assert hip.kv_dtype == "q80" and not hip.fused_rope
    assert hip.k_cache[0].dtype == torch.int8
    assert hip.k_scales[0].dtype == torch.float16
    assert hip.k_scales[0].shape == (hip.k_cache[0].shape[0],
                                     cfg.kv_dim0 // 32)
    return hip


def _paged(models, arch, **kw):
    hip = _hip(models, arch, n_slots=4, kv_pages=KV_PAGES, page_size=P, **kw)
    assert hip.k_cache[0].shape[0] == KV_PAGES * P
    for slot, pages in PAGES_OF.items():
        hip.set_slot_pages(slot, pages)
    return hip


def _check(got, want, arch, what):
    for i in range(len(want)):
        err = _rel_err(got[i], want[i])
        print(f"{arch} {what} row {i}: rel err {err:.5f}")
        assert err < TOL[arch], (arch, what, i, err)
    assert torch.equal(got.argmax(-1), want.argmax(-1)), (arch, what)


def _single(hip, arch, graph):
    """9-token prefill, then 4 decode steps; the logits of all 13 rows."""
    toks = TOKENS[arch][2]
    out = [hip.forward(torch.tensor(toks[:N_PREFILL]),
                       torch.arange(N_PREFILL)).cpu().clone()]
    if graph:
        hip.capture_decode_graph()
    for i in range(N_PREFILL, len(toks)):
        out.append(hip.forward(torch.tensor([toks[i]]),
                               torch.tensor([i])).cpu().clone())
    return torch.cat(out)


@pytest.mark.parametrize("arch", list(TOKENS))
def test_single_sequence_matches_cpu(models, oracle, arch):
    eager = _single(_hip(models, arch), arch, graph=False)
    _check(eager, oracle[arch][2], arch, "eager")
    hip = _hip(models, arch)
    graphed = _single(hip, arch, graph=True)
    assert hip._graph is not None
    assert torch.equal(graphed, eager)


@pytest.mark.parametrize("wide_rows", [False, True])
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("arch", list(TOKENS))
def test_rows_match_cpu(models, oracle, arch, paged, wide_rows):
    """The schedule of tests/test_rows_model.py: mixed prompt chunks and
    decode rows, then all-decode steps, which replay captured graphs and
    equal the eager steps bit for bit."""
    make = _paged if paged else (lambda *a: _hip(*a, n_slots=4))
    got = {}
    for graphs in (False, True):
        hip = make(models, arch)
        hip.set_wide_rows(wide_rows)
        hip.row_graphs = graphs
        got[graphs] = _drive(hip, arch)
        assert bool(hip._row_graphs) == graphs
        assert (hip.attn_splits == 1) == wide_rows
    for s, want in enumerate(oracle[arch]):
        _check(got[True][s], want, arch, f"seq {s}")
        assert torch.equal(got[True][s], got[False][s]), (arch, s)
    if paged:
        # K/V went into the mapped pages and nowhere else
        used = sorted(p for pages in PAGES_OF.values() for p in pages)
        for plane in (hip.k_cache[0], hip.k_scales[0]):
            rows = plane.float().abs().sum(dim=1).reshape(KV_PAGES, P).cpu()
            assert [p for p in range(KV_PAGES) if rows[p].sum() > 0] == used


@pytest.mark.parametrize("arch", ["llama", "qwen3moe"])
def test_force_sync_matches_plain(models, arch):
    """The TP path at world 1 (tests/test_hip_model.py: 0.02, same argmax),
    one sequence and the row schedule."""
    toks = TOKENS[arch][2]
    plain = _hip(models, arch, n_slots=4)
    tp = _hip(models, arch, n_slots=4, force_sync=True)
    t, pos = torch.tensor(toks[:N_PREFILL]), torch.arange(N_PREFILL)
    want = plain.forward(t, pos).cpu().clone()
    got = tp.forward(t, pos).cpu().clone()
    assert _rel_err(got, want) < 0.02, _rel_err(got, want)
    assert torch.equal(got.argmax(-1), want.argmax(-1))
    want = _drive(plain, arch)
    got = _drive(tp, arch)
    for s in range(3):
        err = _rel_err(got[s], want[s])
        print(f"{arch} seq {s}: TP path vs plain rel err {err:.4f}")
        assert err < 0.02, (arch, s, err)


def test_forward_sample_q80(models):
    """The decode graph with the sampler inside, temperature 0: the argmax
    of the logits it leaves."""
    hip = _hip(models, "llama")
    hip.device_sampling = True
    toks = TOKENS["llama"][2]
    hip.forward(torch.tensor(toks[:N_PREFILL]), torch.arange(N_PREFILL))
    hip.capture_decode_graph()
    for i in range(N_PREFILL, len(toks)):
        tok = hip.forward_sample(torch.tensor([toks[i]]), torch.tensor([i]),
                                 0.0, 0.0, 0.9)
        assert tok == int(hip.last_logits().argmax())


def test_kv_cache_bytes_and_dtype_choice(models, monkeypatch):
    from dllama_amd.models.hip_model import HipTransformer
    m, cfg = models["llama"]
    f16 = HipTransformer.from_file(m, cfg, n_slots=2)
    assert f16.kv_dtype == "f16" and not hasattr(f16, "k_scales")
    elems = 2 * cfg.n_layers * 2 * cfg.seq_len * cfg.kv_dim0
    assert f16.kv_cache_bytes() == 2 * elems
    q80 = _hip(models, "llama", n_slots=2)
    assert q80.kv_cache_bytes() == f16.kv_cache_bytes() * 0.53125
    f32 = HipTransformer.from_file(m, cfg, n_slots=2, kv_dtype="f32")
    assert f32.kv_cache_bytes() == 4 * elems
    # the environment picks the default only; an explicit value wins
    monkeypatch.setenv("DLLAMA_KV_F32", "1")
    assert HipTransformer.from_file(m, cfg).kv_dtype == "f32"
    assert HipTransformer.from_file(m, cfg, kv_dtype="f16").k_cache[0].dtype \
        == torch.float16
    _hip(models, "llama")  # asserts q80 planes
    syn = HipTransformer.synthetic(cfg, kv_dtype="q80")
    assert syn.kv_dtype == "q80" and syn.k_cache[0].dtype == torch.int8
    with pytest.raises(ValueError, match="kv_dtype"):
        HipTransformer.from_file(m, cfg, kv_dtype="q4")


def test_gemv_rope_unreachable_with_q80(models):
    """The llama model that takes the GEMV rope epilogue by default runs the
    QKV GEMV + rope_kv pair instead."""
    from dllama_amd.models.hip_model import HipTransformer
    m, cfg = models["llama"]
    assert HipTransformer.from_file(m, cfg).fused_rope
    hip = _hip(models, "llama")
    calls = []
    real = hip.k

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)

    hip.k = Spy()
    hip.forward(torch.tensor([5]), torch.tensor([0]))
    hip.forward(torch.tensor([5, 6, 7]), torch.tensor([1, 2, 3]))
    assert "q40_gemv_rope" not in calls and "rope_kv" in calls
    with pytest.raises(AssertionError):
        hip._gemv_rope(0, hip.layers[0], 1)
