"""Multi-slot CLI and API: `dllama inference --prompt-file --slots N` and
`dllama-api --slots N` give every prompt / request what it gets alone."""

import http.client
import json
import threading

import pytest

from dllama_amd.utils.testing import make_byte_tokenizer, make_tiny_llama

PROMPTS = ["hello world", "abc", "the quick brown fox"]


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    d = tmp_path_factory.mktemp("bapp")
    mp, tp, pf = str(d / "tiny.m"), str(d / "tiny.t"), str(d / "prompts.txt")
    make_byte_tokenizer(tp)
    from dllama_amd.tokenizer import Tokenizer
    vocab = Tokenizer(tp).vocab_size
    make_tiny_llama(mp, vocab_size=vocab + (32 - vocab % 32) % 32)
    with open(pf, "w", encoding="utf-8") as f:
        f.write("\n".join(PROMPTS) + "\n")
    return mp, tp, pf


def _generated(out: str) -> str:
    """What a CLI run printed between its header and its stats block."""
    body = out.split("\nEvaluation")[0]
    return body[body.index("📀"):].split("\n", 1)[1]


def _check_prompt_file(assets, capsys, backend):
    from dllama_amd.apps.main import main
    mp, tp, pf = assets
    common = ["inference", "--model", mp, "--tokenizer", tp, "--steps", "8",
              "--temperature", "0", *backend]
    solo = []
    for p in PROMPTS:
        assert main([*common, "--prompt", p]) == 0
        solo.append(_generated(capsys.readouterr().out))
    assert main([*common, "--prompt-file", pf, "--slots", "2"]) == 0
    out = capsys.readouterr().out
    assert "x 2 slots" in out  # the 📀 line counts every slot's KV
    assert "aggregate" in out.split("Prediction")[1]
    assert _generated(out) == "\n".join(
        f"[{i}] {text}" for i, text in enumerate(solo))
    for p, text in zip(PROMPTS, solo):
        assert text.startswith(p) and len(text) > len(p)


def test_prompt_file_matches_prompt_runs(assets, capsys):
    _check_prompt_file(assets, capsys, ["--gpu-index", "-1"])


@pytest.mark.gpu
def test_prompt_file_matches_prompt_runs_on_gpu(assets, capsys):
    _check_prompt_file(assets, capsys, [])


def _post(port, body):
    conn = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
    conn.request("POST", "/v1/chat/completions", json.dumps(body),
                 {"Content-Type": "application/json"})
    r = conn.getresponse()
    assert r.status == 200
    payload = r.read().decode()
    conn.close()
    if not body.get("stream"):
        data = json.loads(payload)
        assert data["object"] == "chat.completion"
        assert data["usage"]["completion_tokens"] >= 1
        return data["choices"][0]["message"]["content"]
    assert payload.rstrip().endswith("data: [DONE]")
    events = [json.loads(line[6:]) for line in payload.split("\n")
              if line.startswith("data: {")]
    assert all(e["object"] == "chat.completion.chunk" for e in events)
    assert events[-1]["choices"][0]["finish_reason"] == "stop"
    return "".join(e["choices"][0]["delta"].get("content", "")
                   for e in events)


def test_api_two_slots_concurrent_requests(assets):
    from http.server import ThreadingHTTPServer
    from dllama_amd.apps import api as api_mod
    from dllama_amd.apps.main import build_parser
    mp, tp, _ = assets
    port = 18947
    args = build_parser().parse_args(
        ["inference", "--model", mp, "--tokenizer", tp, "--temperature", "0",
         "--seed", "5", "--gpu-index", "-1", "--slots", "2"])
    api_mod.STATE = state = api_mod.ApiState(args)
    sched = state.scheduler
    assert sched is not None
    server = ThreadingHTTPServer(("127.0.0.1", port), api_mod.Handler)
    threading.Thread(target=server.serve_forever, daemon=True).start()
    # A: the server's defaults (greedy), streamed. B: its own temperature
    # and seed, not streamed.
    req_a = {"messages": [{"role": "user", "content": "hi"}],
             "max_tokens": 10, "stream": True}
    req_b = {"messages": [{"role": "user", "content": "tell me more"}],
             "max_tokens": 10, "temperature": 1.5, "seed": 99, "top_p": 0.95}
    try:
        alone_a, alone_b = _post(port, req_a), _post(port, req_b)
        assert _post(port, req_b) == alone_b  # seeded: repeatable

        # hold the scheduler until both requests are queued, so they are
        # certain to share steps
        submitted, both = [], threading.Event()
        real_submit, real_step = sched.submit, sched.engine.step
        peak = []

        def counting_submit(*a):
            real_submit(*a)
            submitted.append(1)
            if len(submitted) == 2:
                both.set()

        def gated_step():
            assert both.wait(30)
            if not sched.inbox.empty():
                return  # let the loop admit the other request first
            peak.append(len(sched.engine.running))
            real_step()

        sched.submit, sched.engine.step = counting_submit, gated_step
        got = {}
        threads = [threading.Thread(
            target=lambda k=k, r=r: got.__setitem__(k, _post(port, r)))
            for k, r in (("a", req_a), ("b", req_b))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(60)
        assert max(peak) == 2
        assert got == {"a": alone_a, "b": alone_b}
    finally:
        server.shutdown()
        server.server_close()
        sched.stop()


def test_api_slots_refused_under_tensor_parallelism(assets, monkeypatch):
    from dllama_amd.apps import api as api_mod
    from dllama_amd.apps import main as main_mod
    from dllama_amd.parallel.comm import SingleComm
    mp, tp, _ = assets

    class TwoRanks(SingleComm):
        world = 2

    monkeypatch.setattr(main_mod, "init_dist_comm", TwoRanks)
    with pytest.raises(SystemExit, match="--slots 2 needs a single GPU"):
        api_mod.main(["--model", mp, "--tokenizer", tp, "--gpu-index", "-1",
                      "--slots", "2"])
