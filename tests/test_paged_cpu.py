"""Paged KV cache on the CPU backend: CpuTransformer with a page table gives
the bits of the unpaged model, refuses rows its table cannot serve, and
BatchEngine over it (page admission, shared prompt prefixes) generates what
every prompt generates alone. Also the --kv-pages options of the apps."""

import http.client
import json
import threading

import pytest
import torch

from dllama_amd import model_file as mf
from dllama_amd.engine import BatchEngine, InferenceEngine
from dllama_amd.models.config import ModelConfig
from dllama_amd.models.cpu_model import CpuTransformer
from dllama_amd.utils.testing import make_byte_tokenizer, make_tiny_llama

P = 4
VOCAB = 256
SEQ_LEN = 48
MAX_TOKENS = 4
# Chosen on the CPU oracle (the model of the `tiny` fixture): at every greedy
# step the top-1/top-2 gap, relative to the largest logit, is above twice the
# HIP tolerance of tests/test_rows_model.py (asserted in _solo). SHARED_A and
# SHARED_B have their first two pages (8 tokens) in common.
TOL = 0.02
PROMPTS = [[65, 253, 233, 137, 252], [39],
           [217, 42, 88, 136, 65, 31, 153, 236, 114]]
GAP = 1e-3  # PROMPTS are those of tests/test_batch_engine.py, with its gap
SHARED_A = [130, 183, 14, 238, 127, 26, 80, 57, 127]
SHARED_B = [130, 183, 14, 238, 127, 26, 80, 57, 143, 93, 199, 81, 36]
OTHER = [2, 107, 110, 84, 85]


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("pg") / "tiny.m")
    make_tiny_llama(p, vocab_size=VOCAB, seq_len=SEQ_LEN, dim=256)
    m = mf.ModelFile(p)
    return m, ModelConfig.from_header(m.header)


class _GapModel:
    """A model proxy recording the top-1/top-2 gap of every logits row a
    token is sampled from, absolute and relative to the largest logit."""

    def __init__(self, model):
        self._m = model
        self.gaps, self.rel_gaps = [], []

    def __getattr__(self, name):
        return getattr(self._m, name)

    def forward(self, tokens, positions):
        logits = self._m.forward(tokens, positions)
        top = torch.topk(logits[-1], 2).values
        self.gaps.append(float(top[0] - top[1]))
        self.rel_gaps.append(float((top[0] - top[1]) / logits[-1].abs().max()))
        return logits


_solo_cache = {}


def solo(tiny, prompt, rel=False):
    """The prompt's greedy run alone on the unpaged model; once per prompt.
    rel: assert the relative gap (the prompts a HIP run is compared on, and
    those whose prefix K/V comes from another step shape), else GAP."""
    key = tuple(prompt)
    if key not in _solo_cache:
        m, cfg = tiny
        model = _GapModel(CpuTransformer(m, cfg))
        out, _ = InferenceEngine(model).generate(prompt, MAX_TOKENS)
        _solo_cache[key] = (out, min(model.gaps), min(model.rel_gaps))
    out, gap, rel_gap = _solo_cache[key]
    if rel:
        assert rel_gap > 2 * TOL, (prompt, rel_gap)
    else:
        assert gap > GAP, (prompt, gap)
    return list(out)


# ------------------------------------------------------------ the model

# 13 rows of three sequences in slots 2, 0 and 3: prompt chunks and decode
# rows mixed, crossing page edges at 4, 8 and 12
SEQS = [[61, 152, 140, 34, 235, 155, 122, 161, 149],
        [17, 156, 4, 215, 67],
        [60, 50, 215, 141, 122, 164, 221, 60, 238, 134, 190, 4, 172]]
SLOT_OF = (2, 0, 3)
SCHEDULE = [[(0, 3), (2, 4), (1, 1)], [(1, 1), (0, 2), (2, 3)],
            [(1, 1), (0, 1), (2, 2)], [(1, 1), (0, 1), (2, 1)],
            [(1, 1), (0, 1), (2, 1)], [(0, 1), (2, 1)], [(2, 1)]]
# slot -> pool pages, scrambled and not monotonic
PAGES_OF = {2: [11, 3, 7], 0: [5, 14], 3: [2, 9, 0, 13]}


def drive(model):
    cursor = [0] * len(SEQS)
    out = []
    for step in SCHEDULE:
        tokens, slots, positions = [], [], []
        for s, n in step:
            for _ in range(n):
                tokens.append(SEQS[s][cursor[s]])
                slots.append(SLOT_OF[s])
                positions.append(cursor[s])
                cursor[s] += 1
        out.append(model.forward_rows(tokens, slots, positions).clone())
    assert cursor == [len(t) for t in SEQS]
    return out


def test_paged_equals_unpaged(tiny):
    m, cfg = tiny
    want = drive(CpuTransformer(m, cfg, n_slots=4))
    paged = CpuTransformer(m, cfg, n_slots=4, kv_pages=16, page_size=P)
    assert paged.k_cache.shape[1] == 16 * P
    for slot, pages in PAGES_OF.items():
        paged.set_slot_pages(slot, pages)
    got = drive(paged)
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    # what was written lies in the mapped pages and nowhere else
    used = sorted(p for pages in PAGES_OF.values() for p in pages)
    rows = paged.k_cache[0].abs().sum(dim=1).reshape(16, P)
    assert [p for p in range(16) if rows[p].sum() > 0] == used


def test_paged_validation(tiny):
    m, cfg = tiny
    with pytest.raises(ValueError, match="page_size"):
        CpuTransformer(m, cfg, n_slots=2, kv_pages=4, page_size=6)
    with pytest.raises(ValueError, match="page_size"):
        CpuTransformer(m, cfg, n_slots=2, kv_pages=4, page_size=2)
    with pytest.raises(ValueError, match="kv_pages=0"):
        CpuTransformer(m, cfg, n_slots=2).set_slot_pages(0, [0])
    model = CpuTransformer(m, cfg, n_slots=3, kv_pages=8, page_size=P)
    with pytest.raises(ValueError, match="rows only"):
        model.forward(torch.tensor([1]), torch.tensor([0]))
    for bad in ([8], [-1], [0, 9]):
        with pytest.raises(ValueError, match="outside the pool"):
            model.set_slot_pages(0, bad)
    with pytest.raises(ValueError, match="slot"):
        model.set_slot_pages(3, [0])
    with pytest.raises(ValueError, match="pages of a sequence"):
        model.set_slot_pages(0, [0], first=SEQ_LEN // P)
    assert model.page_map.users == [0] * 8  # the refused calls mapped nothing
    # nothing mapped: no position can be served
    with pytest.raises(ValueError, match="unmapped"):
        model.forward_rows([1], [0], [0])
    model.set_slot_pages(0, [6])
    model.forward_rows([1], [0], [3])
    with pytest.raises(ValueError, match="unmapped"):
        model.forward_rows([1], [0], [4])   # page 1 of the slot
    # page 2 mapped, page 1 below it not
    model.set_slot_pages(0, [2], first=2)
    with pytest.raises(ValueError, match="unmapped"):
        model.forward_rows([1], [0], [8])
    model.set_slot_pages(0, [1], first=1)
    model.forward_rows([1], [0], [8])
    # slot 1 shares slot 0's first page: reading through it is fine,
    # writing into it is not, from either slot
    model.set_slot_pages(1, [6, 4])
    model.forward_rows([1], [1], [4])
    with pytest.raises(ValueError, match="share"):
        model.forward_rows([1], [1], [3])
    with pytest.raises(ValueError, match="share"):
        model.forward_rows([1], [0], [0])
    model.clear_slot(1)
    model.forward_rows([1], [0], [0])
    assert model.page_map.users == [0, 1, 1, 0, 0, 0, 1, 0]
    # the unpaged checks still stand in front
    with pytest.raises(ValueError, match="two rows"):
        model.forward_rows([1, 2], [0, 0], [1, 1])


def test_shared_pages_at_model_level(tiny):
    """Slot 1 maps slot 0's first two pages and feeds from position 8: the
    logits of feeding everything itself."""
    m, cfg = tiny
    toks = SHARED_B
    model = CpuTransformer(m, cfg, n_slots=2, kv_pages=8, page_size=P)
    model.set_slot_pages(0, [5, 2])
    model.forward_rows(toks[:8], [0] * 8, list(range(8)))
    model.set_slot_pages(1, [5, 2, 7, 0])
    got = model.forward_rows(toks[8:], [1] * 5, list(range(8, 13)))
    fresh = CpuTransformer(m, cfg, n_slots=2, kv_pages=8, page_size=P)
    fresh.set_slot_pages(1, [1, 3, 4, 6])
    want = fresh.forward_rows(toks, [1] * 13, list(range(13)))[8:]
    assert torch.allclose(got, want, atol=1e-6, rtol=1e-4)


# ------------------------------------------------------------ the engine

def _pool_settled(eng):
    pool = eng.pool
    assert all(r == 0 for r in pool.refs)
    assert pool.free + pool.cached == pool.n_pages
    assert all(u == 0 for u in eng.model.page_map.users)
    assert all(p == -1 for row in eng.model.page_map.table for p in row)


def test_engine_waits_for_pages(tiny):
    """Pages for two of the three prompts at most: one waits although a
    slot is free, all finish with their solo tokens."""
    m, cfg = tiny
    need = [-(-(len(p) + MAX_TOKENS) // P) for p in PROMPTS]
    assert need == [3, 2, 4]
    model = CpuTransformer(m, cfg, n_slots=3, kv_pages=6, page_size=P)
    eng = BatchEngine(model)
    seqs = [eng.submit(p, MAX_TOKENS) for p in PROMPTS]
    eng.step()
    assert len(eng.running) == 2 and eng.waiting == [seqs[2]]
    assert len(eng.free_slots) == 1  # a slot was there; the pages were not
    eng.run()
    for prompt, s in zip(PROMPTS, seqs):
        assert s.done and s.tokens == solo(tiny, prompt)
        assert s.stats.cached_tokens == 0
    assert len(eng.free_slots) == 3
    _pool_settled(eng)
    with pytest.raises(ValueError, match="KV pages"):
        eng.submit(list(range(21)), MAX_TOKENS)  # 7 pages, the pool has 6


def test_engine_head_of_queue_is_not_overtaken(tiny):
    m, cfg = tiny
    model = CpuTransformer(m, cfg, n_slots=3, kv_pages=5, page_size=P)
    eng = BatchEngine(model)
    first = eng.submit(PROMPTS[0], MAX_TOKENS)   # 3 pages
    big = eng.submit(PROMPTS[2], MAX_TOKENS)     # 4: does not fit beside it
    small = eng.submit(PROMPTS[1], MAX_TOKENS)   # 2: would fit, must wait
    eng.step()
    assert eng.running == [first] and eng.waiting == [big, small]
    eng.run()
    for prompt, s in zip((PROMPTS[0], PROMPTS[2], PROMPTS[1]),
                         (first, big, small)):
        assert s.tokens == solo(tiny, prompt)
    _pool_settled(eng)


def _run_shared(tiny, share):
    m, cfg = tiny
    model = CpuTransformer(m, cfg, n_slots=3, kv_pages=16, page_size=P)
    eng = BatchEngine(model, share_prefixes=share)
    a = eng.submit(SHARED_A, MAX_TOKENS)
    c = eng.submit(OTHER, MAX_TOKENS)
    eng.run()
    b = eng.submit(SHARED_B, MAX_TOKENS)
    eng.step()
    first_rows = [pos for s, pos in eng.last_step_rows if s is b]
    eng.run()
    return eng, (a, b, c), first_rows


def test_engine_shares_prefix_pages(tiny):
    eng, (a, b, c), first_rows = _run_shared(tiny, share=True)
    assert a.stats.cached_tokens == 0 and c.stats.cached_tokens == 0
    assert b.stats.cached_tokens == 8
    assert first_rows == list(range(8, 13))  # two pages were not stepped
    plain, (a0, b0, c0), rows0 = _run_shared(tiny, share=False)
    assert b0.stats.cached_tokens == 0 and rows0 == list(range(13))
    assert plain.pool.cached == 0
    for s, s0, prompt in ((a, a0, SHARED_A), (b, b0, SHARED_B), (c, c0, OTHER)):
        assert s.tokens == s0.tokens == solo(tiny, prompt, rel=True)
    _pool_settled(eng)
    _pool_settled(plain)
    # generated tokens are registered too: the next turn of A's chat finds
    # every page A filled (12 positions fed: 9 prompt + 3 generated)
    turn2 = eng.submit(SHARED_A + a.tokens, 1)
    eng.run()
    assert turn2.stats.cached_tokens == 12
    _pool_settled(eng)


def test_engine_unpaged_has_no_pool(tiny):
    m, cfg = tiny
    eng = BatchEngine(CpuTransformer(m, cfg, n_slots=2))
    assert eng.pool is None
    s = eng.submit(PROMPTS[0], MAX_TOKENS)
    eng.run()
    assert s.tokens == solo(tiny, PROMPTS[0]) and s.stats.cached_tokens == 0


# ------------------------------------------------------------ the apps

@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    d = tmp_path_factory.mktemp("pgapp")
    mp, tp, pf = str(d / "tiny.m"), str(d / "tiny.t"), str(d / "prompts.txt")
    make_byte_tokenizer(tp)
    from dllama_amd.tokenizer import Tokenizer
    vocab = Tokenizer(tp).vocab_size
    make_tiny_llama(mp, vocab_size=vocab + (32 - vocab % 32) % 32)
    with open(pf, "w", encoding="utf-8") as f:
        f.write("the quick brown fox\nthe quick brown dog\nabc\n")
    return mp, tp, pf


def test_cli_options_and_refusals(assets, monkeypatch):
    from dllama_amd.apps import main as main_mod
    from dllama_amd.parallel.comm import SingleComm
    mp, tp, pf = assets
    args = main_mod.build_parser().parse_args(["inference"])
    assert args.kv_pages == 0 and args.page_size == 64
    common = ["inference", "--model", mp, "--tokenizer", tp, "--gpu-index",
              "-1", "--prompt-file", pf]
    with pytest.raises(SystemExit, match="--kv-pages needs --slots > 1"):
        main_mod.main([*common, "--kv-pages", "8"])
    with pytest.raises(SystemExit, match="--page-size must be a power of two"):
        main_mod.main([*common, "--slots", "2", "--kv-pages", "8",
                       "--page-size", "48"])
    with pytest.raises(SystemExit, match="--kv-pages must be >= 0"):
        main_mod.main([*common, "--slots", "2", "--kv-pages", "-1"])

    class TwoRanks(SingleComm):
        world = 2

    monkeypatch.setattr(main_mod, "init_dist_comm", TwoRanks)
    with pytest.raises(SystemExit, match="--slots 2 needs a single GPU"):
        main_mod.main([*common, "--slots", "2", "--kv-pages", "8"])
    from dllama_amd.apps import api as api_mod
    with pytest.raises(SystemExit, match="needs a single GPU"):
        api_mod.main(["--model", mp, "--tokenizer", tp, "--gpu-index", "-1",
                      "--slots", "2", "--kv-pages", "8"])


def test_cli_prompt_file_paged(assets, capsys):
    from dllama_amd.apps.main import main
    mp, tp, pf = assets
    common = ["inference", "--model", mp, "--tokenizer", tp, "--steps", "6",
              "--temperature", "0", "--gpu-index", "-1", "--prompt-file", pf,
              "--slots", "2"]
    assert main(common) == 0
    plain = capsys.readouterr().out
    assert "nCachedTokens" not in plain
    assert main([*common, "--kv-pages", "24", "--page-size", "4"]) == 0
    out = capsys.readouterr().out
    assert "24 pages x 4 rows shared by 2 slots" in out
    assert "nCachedTokens:" in out
    body = lambda s: s.split("\nEvaluation")[0].split("📀")[1].split("\n", 1)[1]
    assert body(out) == body(plain)


def test_api_reports_cached_tokens(assets):
    from http.server import ThreadingHTTPServer
    from dllama_amd.apps import api as api_mod
    from dllama_amd.apps.main import build_parser
    mp, tp, _ = assets
    port = 18949
    args = build_parser().parse_args(
        ["inference", "--model", mp, "--tokenizer", tp, "--temperature", "0",
         "--seed", "5", "--gpu-index", "-1", "--slots", "2", "--kv-pages",
         "48", "--page-size", "4"])
    api_mod.STATE = state = api_mod.ApiState(args)
    assert state.scheduler.engine.pool is not None
    server = ThreadingHTTPServer(("127.0.0.1", port), api_mod.Handler)
    threading.Thread(target=server.serve_forever, daemon=True).start()

    def post(body):
        conn = http.client.HTTPConnection("127.0.0.1", port, timeout=60)
        conn.request("POST", "/v1/chat/completions", json.dumps(body),
                     {"Content-Type": "application/json"})
        r = conn.getresponse()
        assert r.status == 200
        data = json.loads(r.read().decode())
        conn.close()
        return data

    req = {"messages": [{"role": "user", "content": "hello there"}],
           "max_tokens": 4}
    try:
        first, again = post(req), post(req)
    finally:
        server.shutdown()
        server.server_close()
        state.scheduler.stop()
    n = first["usage"]["prompt_tokens"]
    assert first["usage"]["prompt_tokens_details"] == {"cached_tokens": 0}
    # the same prompt again: every full page but the one holding its last
    # token comes from the first request
    assert again["usage"]["prompt_tokens_details"] == {
        "cached_tokens": (n - 1) // 4 * 4}
    assert (n - 1) // 4 >= 1
