"""Token log-probabilities without a GPU: the oracle (logprob_rows_ref)
against plain numpy float64, the engines on the CPU backend, and the API's
logprobs / top_logprobs fields (stream and not, one slot and two)."""

import http.client
import json
import threading

import numpy as np
import pytest
import torch

from dllama_amd import model_file as mf
from dllama_amd.engine import BatchEngine, InferenceEngine, TokenLogprob
from dllama_amd.models.config import ModelConfig
from dllama_amd.models.cpu_model import CpuTransformer
from dllama_amd.ops.reference import logprob_rows_ref
from dllama_amd.tokenizer import Sampler
from dllama_amd.utils.testing import make_byte_tokenizer, make_tiny_llama


# ------------------------------------------------------------ the oracle

def _numpy_rows(x32, targets, k):
    """The definition, row by row, nothing shared with the oracle: float64
    logsumexp by hand, the order by a python sort on (-value, index)."""
    out = []
    for row, t in zip(np.asarray(x32, dtype=np.float32), targets):
        x = row.astype(np.float64)
        m = x.max()
        lse = m + np.log(np.exp(x - m).sum())
        order = sorted(range(len(row)), key=lambda i: (-float(row[i]), i))[:k]
        out.append((lse, x[t] - lse if 0 <= t < len(row) else -np.inf,
                    [x[i] - lse for i in order], order))
    return out


def _check_ref(x32, targets, k):
    lse, lp, top_lp, top_id = logprob_rows_ref(torch.tensor(x32), targets, k)
    assert lse.dtype == lp.dtype == top_lp.dtype == torch.float64
    assert top_lp.shape == top_id.shape == (len(x32), 20)
    for b, (w_lse, w_lp, w_top, w_order) in enumerate(
            _numpy_rows(x32, targets, k)):
        n = len(w_order)
        assert abs(float(lse[b]) - w_lse) < 1e-12
        assert float(lp[b]) == w_lp or abs(float(lp[b]) - w_lp) < 1e-12
        assert top_id[b, :n].tolist() == w_order
        assert top_id[b, n:].tolist() == [-1] * (20 - n)
        np.testing.assert_allclose(top_lp[b, :n].numpy(), w_top, atol=1e-12)
        assert (top_lp[b, n:] == float("-inf")).all()


def test_ref_matches_numpy():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((3, 300)) * 3).astype(np.float32)
    _check_ref(x, [0, 299, 17], 5)
    _check_ref(x, [5, 6, 7], 0)
    _check_ref(x + 1e4, [1, 2, 3], 20)


def test_ref_ties_lower_index_first():
    x = np.zeros((2, 40), dtype=np.float32)
    x[0, [3, 9, 30]] = 2.5            # three equal maxima
    x[1, 7], x[1, 2] = -0.0, 0.0      # -0.0 equals +0.0: index decides
    x[1, 8:] = -1.0
    _check_ref(x, [9, 7], 20)
    _, _, _, ids = logprob_rows_ref(torch.tensor(x), [9, 7], 4)
    assert ids[0, :4].tolist() == [3, 9, 30, 0]
    assert ids[1, :4].tolist() == [0, 1, 2, 3]


def test_ref_k_beyond_vocab_and_missing_target():
    x = np.arange(7, dtype=np.float32)[None].repeat(3, 0)
    _check_ref(x, [-1, 7, 6], 20)
    lse, lp, top_lp, top_id = logprob_rows_ref(torch.tensor(x), [-1, 7, 6], 20)
    assert lp[0] == lp[1] == float("-inf") and lp[2] == top_lp[2, 0]
    assert top_id[0].tolist() == [6, 5, 4, 3, 2, 1, 0] + [-1] * 13
    with pytest.raises(ValueError):
        logprob_rows_ref(torch.tensor(x), [0, 0, 0], 21)


# ------------------------------------------------------------ the engines

@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("lp") / "tiny.m")
    make_tiny_llama(p, vocab_size=256)
    m = mf.ModelFile(p)
    return m, ModelConfig.from_header(m.header)


PROMPT = [3, 17, 101]


def test_generate_entries_match_the_reference(tiny):
    plain, _ = InferenceEngine(CpuTransformer(*tiny),
                               sampler=Sampler(256, 0.8, 0.9, 11)).generate(PROMPT, 6)
    seen, called = [], []
    out, stats = InferenceEngine(
        CpuTransformer(*tiny), sampler=Sampler(256, 0.8, 0.9, 11)).generate(
            PROMPT, 6, on_token=lambda t: seen.append(("t", t)), logprobs=3,
            on_logprobs=lambda e: (seen.append(("e", e.token)), called.append(e)))
    assert out == plain  # the tokens do not depend on the setting
    assert called == stats.logprobs and len(stats.logprobs) == len(out) == 6
    # on_logprobs right after on_token, for the same token
    assert seen == [(kind, t) for t in out for kind in ("t", "e")]
    # the reference on decode_one's logits of a model fed the same tokens
    eng = InferenceEngine(CpuTransformer(*tiny))
    logits = eng.prefill(PROMPT)
    for token, entry in zip(out, stats.logprobs):
        assert isinstance(entry, TokenLogprob) and entry.token == token
        _, lp, top_lp, top_id = logprob_rows_ref(logits, [token], 3)
        assert entry.logprob == float(lp[0]) <= 0.0
        assert entry.top == list(zip(top_id[0, :3].tolist(),
                                     top_lp[0, :3].tolist()))
        assert entry.top[0][1] >= entry.logprob
        logits = eng.decode_one(token)
    assert InferenceEngine(CpuTransformer(*tiny)).generate(PROMPT, 2)[1].logprobs is None
    with pytest.raises(ValueError):
        InferenceEngine(CpuTransformer(*tiny)).generate(PROMPT, 2, logprobs=21)


def test_batch_engine_only_the_asking_sequence(tiny):
    alone = BatchEngine(CpuTransformer(*tiny, n_slots=2))
    want = alone.generate_many([PROMPT, [5, 6]], 5)
    eng = BatchEngine(CpuTransformer(*tiny, n_slots=2))
    got = []
    a = eng.submit(PROMPT, 5, logprobs=2, on_logprobs=got.append)
    b = eng.submit([5, 6], 5)
    eng.run()
    assert [a.tokens, b.tokens] == [w[0] for w in want]
    assert b.stats.logprobs is None
    assert got == a.stats.logprobs and len(got) == 5
    assert [e.token for e in got] == a.tokens
    # against a single-sequence run of the same prompt
    _, stats = InferenceEngine(CpuTransformer(*tiny)).generate(PROMPT, 5, logprobs=2)
    for e, w in zip(got, stats.logprobs):
        assert e.token == w.token and len(e.top) == 2
        assert e.logprob == pytest.approx(w.logprob, abs=1e-4)
        assert [i for i, _ in e.top] == [i for i, _ in w.top]


# ------------------------------------------------------------ the API

@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    d = tmp_path_factory.mktemp("lpapi")
    mp, tp = str(d / "tiny.m"), str(d / "tiny.t")
    make_byte_tokenizer(tp)
    from dllama_amd.tokenizer import Tokenizer
    vocab = Tokenizer(tp).vocab_size
    make_tiny_llama(mp, vocab_size=vocab + (32 - vocab % 32) % 32)
    return mp, tp


def _serve(assets, port, slots):
    from http.server import HTTPServer, ThreadingHTTPServer
    from dllama_amd.apps import api as api_mod
    from dllama_amd.apps.main import build_parser
    mp, tp = assets
    argv = ["inference", "--model", mp, "--tokenizer", tp, "--temperature", "0",
            "--seed", "5", "--gpu-index", "-1", "--port", str(port)]
    if slots > 1:
        argv += ["--slots", str(slots)]
    api_mod.STATE = state = api_mod.ApiState(build_parser().parse_args(argv))
    server = (ThreadingHTTPServer if slots > 1 else HTTPServer)(
        ("127.0.0.1", port), api_mod.Handler)
    threading.Thread(target=server.serve_forever, daemon=True).start()
    return state, server


def _post(port, body):
    conn = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    conn.request("POST", "/v1/chat/completions", json.dumps(body),
                 {"Content-Type": "application/json"})
    r = conn.getresponse()
    payload = r.read().decode()
    conn.close()  # keep-alive would block the single-threaded server loop
    return r.status, payload


def _events(payload):
    assert payload.rstrip().endswith("data: [DONE]")
    return [json.loads(line[6:]) for line in payload.split("\n")
            if line.startswith("data: {")]


def _check_content(content, top):
    for e in content:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
        assert bytes(e["bytes"]).decode("utf-8", errors="replace") == e["token"]
        assert -9999.0 <= e["logprob"] <= 0.0
        assert len(e["top_logprobs"]) == top
        for alt in e["top_logprobs"]:
            assert set(alt) == {"token", "logprob", "bytes"}
            assert bytes(alt["bytes"]).decode("utf-8", errors="replace") == alt["token"]
        lps = [alt["logprob"] for alt in e["top_logprobs"]]
        assert lps == sorted(lps, reverse=True)
        if top:
            assert lps[0] >= e["logprob"]
            if e["logprob"] == lps[0]:  # greedy: the token leads its own list
                assert e["top_logprobs"][0]["bytes"] == e["bytes"]


@pytest.mark.parametrize("slots,port", [(1, 18961), (2, 18962)])
def test_api_logprobs(assets, slots, port):
    state, server = _serve(assets, port, slots)
    msg = [{"role": "user", "content": "hi"}]
    try:
        # not streamed; max_tokens ends it, so every token is listed
        status, payload = _post(port, {"messages": msg, "max_tokens": 6,
                                       "logprobs": True, "top_logprobs": 3})
        assert status == 200
        data = json.loads(payload)
        content = data["choices"][0]["logprobs"]["content"]
        n_gen = data["usage"]["completion_tokens"]
        _check_content(content, 3)
        # the final-token rule: a token that ended the generation (an EOS id
        # or the end of a stop string) is not listed, every other one is
        assert len(content) in (n_gen, n_gen - 1)
        text = data["choices"][0]["message"]["content"]
        if len(content) == n_gen:
            assert n_gen == 6
        listed = b"".join(bytes(e["bytes"]) for e in content)
        assert listed.decode("utf-8", errors="replace").startswith(text)

        # logprobs without top_logprobs: empty lists
        status, payload = _post(port, {"messages": msg, "max_tokens": 3,
                                       "logprobs": True})
        assert status == 200
        _check_content(json.loads(payload)["choices"][0]["logprobs"]["content"], 0)

        # streamed: the same entries, spread over the chunks that released
        # their text
        status, payload = _post(port, {"messages": msg, "max_tokens": 6,
                                       "stream": True, "logprobs": True,
                                       "top_logprobs": 3})
        assert status == 200
        events = _events(payload)
        streamed = [e for ev in events[:-1]
                    for e in ev["choices"][0]["logprobs"]["content"]]
        assert "logprobs" not in events[-1]["choices"][0]
        # (the prompt's cached prefix is not stepped again, so the logits
        # differ in the last bits between the two requests)
        assert [e["bytes"] for e in streamed] == [e["bytes"] for e in content]
        assert ([e["logprob"] for e in streamed]
                == pytest.approx([e["logprob"] for e in content], abs=1e-4))
        _check_content(streamed, 3)
        assert "".join(ev["choices"][0]["delta"].get("content", "")
                       for ev in events) == text

        # refused
        for bad in ({"logprobs": True, "top_logprobs": 21},
                    {"top_logprobs": 2},
                    {"logprobs": False, "top_logprobs": 2},
                    {"logprobs": True, "top_logprobs": -1}):
            status, payload = _post(port, {"messages": msg, "max_tokens": 2, **bad})
            assert status == 400, bad
            err = json.loads(payload)["error"]
            assert err["type"] == "invalid_request_error"
            assert err["param"] == "top_logprobs" and err["message"]

        # without the field: no logprobs key anywhere
        status, payload = _post(port, {"messages": msg, "max_tokens": 6})
        assert status == 200
        plain = json.loads(payload)
        assert "logprobs" not in plain["choices"][0]
        assert plain["choices"][0]["message"]["content"] == text
        status, payload = _post(port, {"messages": msg, "max_tokens": 4,
                                       "stream": True})
        assert all("logprobs" not in ev["choices"][0] for ev in _events(payload))
    finally:
        server.shutdown()
        server.server_close()
        if state.scheduler is not None:
            state.scheduler.stop()


def test_api_final_token_is_not_listed(assets):
    """The _Deltas rule on its own: an EOS id, and the token that completes
    a stop string, are not listed; tokens held back as a possible stop
    string go with the delta that releases them."""
    from dllama_amd.apps.api import _Deltas
    from dllama_amd.tokenizer import EosDetector, Tokenizer
    tok = Tokenizer(assets[1])
    eos = tok.eos_token_ids[0]
    a, b, c, d = (ord(ch) for ch in "aXYb")

    def run(tokens, stops):
        got = []
        tok.reset_decoder()
        s = _Deltas(tok, EosDetector(tok.eos_token_ids, stops),
                    lambda delta, entries: got.append(
                        (delta, [bytes(e["bytes"]) for e in entries])), True)
        for t in tokens:
            s.on_token(t)
            s.on_logprobs(TokenLogprob(t, float("-inf"), [(t, -0.5)]))
        s.finish()
        return got, s

    got, s = run([a, eos], [])
    assert got == [("a", [b"a"])]
    # "XY" is the stop string: X is held, Y completes it and is not listed
    got, _ = run([a, b, c], ["XY"])
    assert got == [("a", [b"a"]), ("", [b"X"])]
    # X held, then b shows it was not the stop string: both go with "Xb"
    got, _ = run([a, b, d], ["XY"])
    assert got == [("a", [b"a"]), ("Xb", [b"X", b"b"])]
    # max_tokens ends it while X is held: listed with an empty delta
    got, _ = run([a, b], ["XY"])
    assert got == [("a", [b"a"]), ("", [b"X"])]
    # -inf is sent as -9999.0
    entry = s._json(TokenLogprob(a, float("-inf"), [(b, -0.25)]))
    assert entry["logprob"] == -9999.0
    assert entry["top_logprobs"] == [{"token": "X", "logprob": -0.25,
                                      "bytes": [ord("X")]}]
