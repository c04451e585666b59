"""set_logprobs on HipTransformer, and what sits on it: the engines, the
API field and `dllama perplexity`, on the GPU.

Every comparison is with logprob_rows_ref applied to the HIP model's own
last_logits() / rows_logits(), never to another backend's logits, so no
near-tie between backends can enter. Bounds: ids exactly, values within the
2e-5 of tests/test_logprob_ops.py (tiny vocabularies, |lse| < 16)."""

import http.client
import json
import threading

import numpy as np
import pytest
import torch

from dllama_amd import model_file as mf
from dllama_amd.engine import BatchEngine, InferenceEngine
from dllama_amd.models.config import ModelConfig
from dllama_amd.ops.reference import logprob_rows_ref
from dllama_amd.tokenizer import Sampler
from dllama_amd.utils.testing import (make_byte_tokenizer, make_tiny_llama,
                                      make_tiny_qwen3)

pytestmark = pytest.mark.gpu

TOL = 2e-5
PROMPT = [3, 17, 101]
T, TOPP = 0.8, 0.9


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("lpm")
    out = {}
    for arch in ("llama", "qwen3"):
        p = str(d / f"{arch}.m")
        if arch == "llama":
            make_tiny_llama(p, vocab_size=256)
        else:
            make_tiny_qwen3(p, moe=False)
        m = mf.ModelFile(p)
        out[arch] = (m, ModelConfig.from_header(m.header))
    return out


def _model(models, arch="llama", device_sampling=True, **kw):
    from dllama_amd.models.hip_model import HipTransformer
    model = HipTransformer.from_file(*models[arch], **kw)
    model.device_sampling = device_sampling
    return model


def _matches(result, row, token):
    """One row's (lse, logprob, top_ids, top_logprobs) against the oracle on
    that row's own logits."""
    lse, lp, ids, lps = result
    w_lse, w_lp, w_top, w_id = logprob_rows_ref(row, [token], 20)
    assert len(ids) == len(lps) == 20
    assert ids == w_id[0].tolist()
    assert abs(lse - float(w_lse[0])) <= TOL
    assert abs(lp - float(w_lp[0])) <= TOL
    assert np.abs(np.array(lps) - w_top[0].numpy()).max() <= TOL
    assert lp <= 0.0 and lps[0] >= lp


def _decode(model, steps, temp, topp, seed=4321, check=True):
    """forward_sample from position 3 on; every step's last_logprobs() is
    checked against the row the step left."""
    coins = Sampler(256, T, TOPP, seed)
    token, out = 7, []
    for i in range(steps):
        coin = coins.next_coin()
        token = model.forward_sample(torch.tensor([token]),
                                     torch.tensor([3 + i]), coin, temp, topp)
        assert token is not None
        if check:
            _matches(model.last_logprobs(), model.last_logits().clone(), token)
        out.append(token)
    return out


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("temp,topp", [(0.0, 0.9), (T, TOPP)])
def test_forward_sample(models, graph, temp, topp):
    model = _model(models)
    model.forward(torch.tensor(PROMPT), torch.arange(3))
    model.set_logprobs(True)
    if graph:
        model.capture_decode_graph()
        assert model._graph_samples
        eager = []
        k = model.k

        class Counting:
            def __getattr__(self, name):
                if name in ("sample_logits", "logprob_rows"):
                    eager.append(name)
                return getattr(k, name)
        model._sampler().k = model.k = Counting()
    out = _decode(model, 4, temp, topp)
    if graph:
        assert not eager  # sampler and logprob_rows ran inside the replays
    # sample_row reports the same row the same way
    row = model.last_logits().clone()
    token = model.sample_row(row, 0.5, temp, topp)
    _matches(model.last_logprobs(), row, token)
    if temp == 0.0:
        assert token == out[-1] == int(row.argmax())
        assert model.last_logprobs()[2][0] == token


def test_same_tokens_on_and_off(models):
    off = _model(models)
    on = _model(models)
    for m in (off, on):
        m.forward(torch.tensor(PROMPT), torch.arange(3))
        m.capture_decode_graph()
    on.set_logprobs(True)
    assert _decode(on, 12, T, TOPP) == _decode(off, 12, T, TOPP, check=False)


def test_graphs_of_both_settings_are_kept(models):
    model = _model(models)
    model.forward(torch.tensor(PROMPT), torch.arange(3))
    model.capture_decode_graph()
    g_off = model._graph
    first = _decode(model, 2, T, TOPP, check=False)
    model.set_logprobs(True)
    model.forward_sample(torch.tensor([first[-1]]), torch.tensor([5]), 0.3, T, TOPP)
    g_on = model._graph
    assert g_on is not None and g_on is not g_off and model._graph_samples
    model.set_logprobs(False)
    assert model._graph is g_off and model._graph_samples
    # a request without logprobs between two with: nothing is recaptured
    model.forward_sample(torch.tensor([9]), torch.tensor([6]), 0.3, T, TOPP)
    assert model._graph is g_off
    model.set_logprobs(True)
    assert model._graph is g_on
    # a split change drops the graphs of both settings
    model._set_attn_splits(16)
    assert model._graph is not g_on
    model.set_logprobs(False)
    assert model._graph is None  # recaptured when the next step needs it
    tok = model.forward_sample(torch.tensor([9]), torch.tensor([7]), 0.3, T, TOPP)
    assert model._graph is not None and model._graph is not g_off
    assert tok is not None


def _rows_steps(model, arch="llama"):
    """A mixed step with a prompt chunk (eager), then all-decode steps of
    B = 3 rows (captured, then replayed); every row of every step checked."""
    steps = [([3, 17, 50, 9], [2, 2, 3, 0], [0, 1, 0, 0]),
             ([101, 51, 10], [2, 3, 0], [2, 1, 1]),
             ([7, 52, 11], [2, 3, 0], [3, 2, 2]),
             ([8, 53, 12], [2, 3, 0], [4, 3, 3])]
    coins = Sampler(256, T, TOPP, 77)
    for tokens, slots, positions in steps:
        B = len(tokens)
        cs = [coins.next_coin() for _ in range(B)]
        temps = [0.0 if b % 2 else T for b in range(B)]
        picked = model.forward_rows_sample(tokens, slots, positions, cs, temps,
                                           [TOPP] * B)
        rows = model.rows_logits(B).clone()
        results = model.rows_logprobs(B)
        assert len(results) == B and None not in picked
        for b in range(B):
            _matches(results[b], rows[b], picked[b])
            if temps[b] == 0.0:
                assert picked[b] == int(rows[b].argmax()) == results[b][2][0]


@pytest.mark.parametrize("arch", ["llama", "qwen3"])
def test_forward_rows_sample(models, arch):
    model = _model(models, arch, n_slots=4)
    model.set_logprobs(True)
    _rows_steps(model)
    assert list(model._row_graphs) == [3]
    g_on = model._row_graphs[3]
    model.set_logprobs(False)
    assert model._row_graphs.get(3) is None  # the off setting has its own
    model.set_logprobs(True)
    assert model._row_graphs.get(3) is g_on


def test_rows_paged(models):
    model = _model(models, n_slots=4, kv_pages=8, page_size=4)
    for slot, pages in ((0, [0, 1]), (2, [2, 3]), (3, [4, 5])):
        model.set_slot_pages(slot, pages)
    model.set_logprobs(True)
    _rows_steps(model)


def test_rows_kv_q80(models):
    model = _model(models, n_slots=4, kv_dtype="q80")
    model.set_logprobs(True)
    _rows_steps(model)


def test_tp_path_world1(models):
    """The gathered row of the tp_path is read with its own stride. Against
    its own logits the usual bound; against the plain model the bound of the
    Q80 sync (tests/test_hip_model.py: logits within 2% of the largest), as
    a difference of two logits: 2 * 0.02 * max |logit|."""
    plain, tp = _model(models), _model(models, force_sync=True)
    assert tp.tp_path
    got = {}
    for name, m in (("plain", plain), ("tp", tp)):
        m.forward(torch.tensor(PROMPT), torch.arange(3))
        m.capture_decode_graph()
        m.set_logprobs(True)
        _decode(m, 1, 0.0, TOPP)
        got[name] = (m.last_logprobs(), float(m.last_logits().abs().max()))
    (p, scale), (t, _) = got["plain"], got["tp"]
    assert p[2][0] == t[2][0]
    assert abs(p[1] - t[1]) <= 0.04 * scale
    assert abs(p[0] - t[0]) <= 0.04 * scale
    # rows through the tp_path: logits_full has the row stride world * vocab0
    rows = _model(models, n_slots=4, force_sync=True)
    rows.set_logprobs(True)
    _rows_steps(rows)


def test_logprob_targets_prefill_chunk(models):
    """32 rows of a prefill chunk against the host formula of
    run_perplexity (row - logsumexp(row), float32 on the host)."""
    model = _model(models)
    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(0, 256, (33,), generator=g).tolist()
    logits = model.forward(torch.tensor(tokens[:32]), torch.arange(32))
    targets = tokens[1:32] + [-1]
    got = model.logprob_targets(logits, targets)
    host = logits.detach().float().cpu()
    assert len(got) == 32 and got[-1] == float("-inf")
    for j in range(31):
        want = float((host[j] - torch.logsumexp(host[j], dim=-1))[targets[j]])
        assert abs(got[j] - want) <= TOL, (j, got[j], want)


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    d = tmp_path_factory.mktemp("lpapp")
    mp, tp = str(d / "tiny.m"), str(d / "tiny.t")
    make_byte_tokenizer(tp)
    from dllama_amd.tokenizer import Tokenizer
    vocab = Tokenizer(tp).vocab_size
    make_tiny_llama(mp, vocab_size=vocab + (32 - vocab % 32) % 32)
    return mp, tp


def test_perplexity_cli(assets, capsys, monkeypatch):
    """`dllama perplexity` on the HIP backend prints what the old host
    formula gives on the same logits, and copies no [B, vocab] block."""
    from dllama_amd.apps.main import main
    from dllama_amd.models.hip_model import HipTransformer
    from dllama_amd.tokenizer import Tokenizer
    mp, tp = assets
    text = "the quick brown fox jumps over the lazy dog and hello world " * 2
    seen = []
    real = HipTransformer.logprob_targets
    monkeypatch.setattr(HipTransformer, "logprob_targets",
                        lambda self, logits, t: (seen.append(
                            (logits.detach().float().cpu(), list(t))),
                            real(self, logits, t))[1])
    assert main(["perplexity", "--model", mp, "--tokenizer", tp,
                 "--prompt", text]) == 0
    out = capsys.readouterr().out
    ppl = float(out.split("Perplexity:")[1].split()[0])
    tokens = Tokenizer(tp).encode(text)
    assert len(tokens) > 33 and len(seen) == -(-(len(tokens) - 1) // 32)
    nll, count = 0.0, 0
    for logits, targets in seen:  # the formula run_perplexity had
        for row, t in zip(logits, targets):
            if t >= 0:
                nll -= float((row - torch.logsumexp(row, dim=-1))[t])
                count += 1
    assert count == len(tokens) - 1
    assert ppl == pytest.approx(float(np.exp(nll / count)), rel=1e-4)


def test_engines_on_gpu(models):
    # InferenceEngine: same tokens with and without, entries per token
    def engine():
        m = _model(models)
        m.capture_decode_graph()
        return InferenceEngine(m, sampler=Sampler(256, T, TOPP, 5))
    plain, _ = engine().generate(PROMPT, 8)
    eng = engine()
    out, stats = eng.generate(PROMPT, 8, logprobs=2)
    assert out == plain and not eng.model.logprobs
    assert [e.token for e in stats.logprobs] == out
    # BatchEngine: two sequences, one asking
    model = _model(models, n_slots=2)
    be = BatchEngine(model)
    a = be.submit(PROMPT, 6, Sampler(256, T, TOPP, 5), logprobs=2)
    b = be.submit([5, 6], 6, Sampler(256, T, TOPP, 6))
    be.run()
    assert b.stats.logprobs is None and not model.logprobs
    assert [e.token for e in a.stats.logprobs] == a.tokens and len(a.tokens) == 6
    for e in a.stats.logprobs + stats.logprobs:
        assert len(e.top) == 2 and e.logprob <= 0.0
        assert e.top[0][1] >= e.logprob >= -50.0
        assert e.top[0][1] >= e.top[1][1]


def test_api_request_on_gpu(assets):
    from http.server import HTTPServer
    from dllama_amd.apps import api as api_mod
    from dllama_amd.apps.main import build_parser
    mp, tp = assets
    port = 18971
    args = build_parser().parse_args(
        ["inference", "--model", mp, "--tokenizer", tp, "--temperature", "0.8",
         "--seed", "5", "--port", str(port)])
    api_mod.STATE = api_mod.ApiState(args)
    server = HTTPServer(("127.0.0.1", port), api_mod.Handler)
    threading.Thread(target=server.serve_forever, daemon=True).start()
    try:
        conn = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        conn.request("POST", "/v1/chat/completions", json.dumps(
            {"messages": [{"role": "user", "content": "hi"}], "max_tokens": 8,
             "logprobs": True, "top_logprobs": 2}),
            {"Content-Type": "application/json"})
        r = conn.getresponse()
        assert r.status == 200
        data = json.loads(r.read())
        conn.close()
        content = data["choices"][0]["logprobs"]["content"]
        n_gen = data["usage"]["completion_tokens"]
        assert len(content) in (n_gen, n_gen - 1) and content
        for e in content:
            assert e["logprob"] <= 0.0 and len(e["top_logprobs"]) == 2
            assert e["top_logprobs"][0]["logprob"] >= e["logprob"]
            assert bytes(e["bytes"]).decode("utf-8", errors="replace") == e["token"]
    finally:
        server.shutdown()
        server.server_close()
