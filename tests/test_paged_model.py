"""HipTransformer with a paged KV cache: the row steps of
tests/test_rows_model.py with every slot's rows scattered over a page pool
(page_size 4: the 13-token lists cross three page edges), against the CPU
oracle, against the unpaged model, with shared prefix pages, and under a
BatchEngine."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd import model_file as mf
from dllama_amd.engine import BatchEngine
from dllama_amd.models.config import ModelConfig
from dllama_amd.models.cpu_model import CpuTransformer
from dllama_amd.utils.testing import make_tiny_llama, make_tiny_qwen3

from test_paged_cpu import (MAX_TOKENS, OTHER, SEQ_LEN, SHARED_A, SHARED_B,
                            VOCAB, _pool_settled, solo)
from test_rows_model import SCHEDULE, SLOT_OF, TOKENS, TOL, _drive, _rel_err

P = 4
# slot -> pool pages, scrambled and not monotonic (slots as SLOT_OF: the
# 9-, 5- and 13-token sequences live in slots 2, 0 and 3)
PAGES_OF = {2: [11, 3, 7], 0: [5, 14], 3: [2, 9, 0, 13]}
KV_PAGES = 16


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("paged")
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
    """Per arch: the CPU logits of every sequence run alone, with the
    top-1/top-2 gap of every row above twice the tolerance. Computed once,
    shared, never written."""
    out = {}
    for arch, (m, cfg) in models.items():
        rows = []
        for toks in TOKENS[arch]:
            want = CpuTransformer(m, cfg).forward(torch.tensor(toks),
                                                  torch.arange(len(toks)))
            top = torch.topk(want, 2).values
            gap = (top[:, 0] - top[:, 1]) / want.abs().max(dim=1).values
            assert gap.min().item() > 2 * TOL[arch], (arch, gap)
            rows.append(want)
        out[arch] = rows
    return out


def _hip(models, arch, **kw):
    from dllama_amd.models.hip_model import HipTransformer
    m, cfg = models[arch]
    return HipTransformer.from_file(m, cfg, **kw)


def _paged(models, arch, **kw):
    hip = _hip(models, arch, n_slots=4, kv_pages=KV_PAGES, page_size=P, **kw)
    assert hip.k_cache[0].shape[0] == KV_PAGES * P
    for slot, pages in PAGES_OF.items():
        hip.set_slot_pages(slot, pages)
    return hip


@pytest.mark.parametrize("arch", list(TOKENS))
def test_paged_matches_cpu(models, oracle, arch):
    hip = _paged(models, arch)
    got = _drive(hip, arch)
    for s, (g, want) in enumerate(zip(got, oracle[arch])):
        for i in range(len(want)):
            err = _rel_err(g[i], want[i])
            print(f"{arch} seq {s} row {i}: rel err {err:.5f}")
            assert err < TOL[arch], (arch, s, i, err)
        assert torch.equal(g.argmax(-1), want.argmax(-1)), (arch, s)
    # K/V went into the mapped pages and nowhere else
    used = sorted(p for pages in PAGES_OF.values() for p in pages)
    rows = hip.k_cache[0].float().abs().sum(dim=1).reshape(KV_PAGES, P).cpu()
    assert [p for p in range(KV_PAGES) if rows[p].sum() > 0] == used


@pytest.mark.parametrize("arch", list(TOKENS))
def test_paged_matches_unpaged(models, arch):
    """The same launches on the same values, through other addresses; the
    all-decode steps replay one captured graph and the page table is sent
    once per mapped slot, never during the replays."""
    prefill = [[(0, 5), (1, 1), (2, 9)]]
    decode = [[(1, 1), (0, 1), (2, 1)]] * 4
    want = _drive(_hip(models, arch, n_slots=4), arch, prefill + decode)
    hip = _paged(models, arch)
    assert hip.page_table_sends == 0  # nothing is sent before a step needs it
    sends = []
    run = hip._run_rows

    def counting_run(*a, **kw):
        sends.append(hip.page_table_sends)
        return run(*a, **kw)

    hip._run_rows = counting_run
    got = _drive(hip, arch, prefill + decode)
    assert list(hip._row_graphs) == [3]
    assert sends == [3] * 5 and hip.page_table_sends == 3
    for s in range(3):
        err = _rel_err(got[s], want[s])
        print(f"{arch} seq {s}: paged vs unpaged rel err {err:.2e}")
        assert err < 1e-5, (arch, s, err)
    pps = hip.page_map.pages_per_seq
    assert hip.rows[:3, 0].tolist() == [0 * pps, 2 * pps, 3 * pps]
    assert hip.rows[:3, 1].tolist() == [5, 9, 13]
    table = hip.page_table.cpu()
    assert table[2, :3].tolist() == PAGES_OF[2] and not table[1].any()
    assert int(table.max()) < KV_PAGES and int(table.min()) >= 0


@pytest.mark.parametrize("arch", list(TOKENS))
def test_shared_prefix_pages(models, arch):
    """Slot 0 feeds 8 tokens; slot 1 maps slot 0's first two pages plus its
    own and feeds from position 8: the logits of a fresh model whose slot 1
    feeds everything itself (the prefix K/V came from another launch
    shape: the composition-invariance bound)."""
    toks = TOKENS[arch][2]
    hip = _hip(models, arch, n_slots=2, kv_pages=8, page_size=P)
    hip.set_slot_pages(0, [5, 2])
    hip.forward_rows(toks[:8], [0] * 8, list(range(8)))
    hip.set_slot_pages(1, [5, 2, 7, 0])
    got = [hip.forward_rows(toks[8:11], [1] * 3, [8, 9, 10]).cpu().clone()]
    got += [hip.forward_rows([toks[i]], [1], [i]).cpu().clone()
            for i in (11, 12)]
    fresh = _hip(models, arch, n_slots=2, kv_pages=8, page_size=P)
    fresh.set_slot_pages(1, [1, 3, 4, 6])
    want = [fresh.forward_rows(toks[:11], [1] * 11, list(range(11))).cpu()[8:]
            .clone()]
    want += [fresh.forward_rows([toks[i]], [1], [i]).cpu().clone()
             for i in (11, 12)]
    err = _rel_err(torch.cat(got), torch.cat(want))
    print(f"{arch}: shared prefix pages vs own rel err {err:.2e}")
    assert err < 1e-4, err


def test_paged_validation_before_any_launch(models):
    hip = _hip(models, "llama", n_slots=3, kv_pages=8, page_size=P)
    with pytest.raises(ValueError, match="outside the pool"):
        hip.set_slot_pages(0, [8])
    hip.set_slot_pages(0, [6])
    hip.set_slot_pages(1, [6, 4])
    hip.set_slot_pages(2, [1], first=1)
    hip.k = None  # a launch, or a lookup of one, would be an AttributeError
    for call in (lambda: hip.forward(torch.tensor([1]), torch.tensor([0])),
                 lambda: hip.forward_sample(torch.tensor([1]),
                                            torch.tensor([0]), 0.0, 0.0, 0.9),
                 hip.capture_decode_graph):
        with pytest.raises(ValueError, match="rows only"):
            call()
    with pytest.raises(ValueError, match="unmapped"):
        hip.forward_rows([1], [0], [4])       # page 1 of slot 0
    with pytest.raises(ValueError, match="unmapped"):
        hip.forward_rows([1], [2], [4])       # page 0 below it is unmapped
    with pytest.raises(ValueError, match="share"):
        hip.forward_rows([1], [1], [3])       # page 6 is slot 0's too
    with pytest.raises(ValueError, match="share"):
        hip.forward_rows([1, 2], [1, 0], [4, 0])
    with pytest.raises(ValueError, match="share"):
        hip.forward_rows_sample([1], [0], [0], [0.0], [0.0], [0.9])
    assert hip._rows_io is None and hip.page_table_sends == 0  # nothing staged
    with pytest.raises(ValueError, match="kv_pages=0"):
        _hip(models, "llama", n_slots=2).set_slot_pages(0, [0])
    with pytest.raises(ValueError, match="page_size"):
        _hip(models, "llama", n_slots=2, kv_pages=4, page_size=12)


def test_batch_engine_paged_matches_cpu_solo(tmp_path):
    """BatchEngine on the paged HIP model: the tokens of the CPU solo runs
    (gaps asserted on the oracle in solo), the second prompt's first two
    pages taken from the first one's, every page free or cached at the
    end."""
    from dllama_amd.models.hip_model import HipTransformer
    p = str(tmp_path / "tiny.m")
    make_tiny_llama(p, vocab_size=VOCAB, seq_len=SEQ_LEN, dim=256)
    m = mf.ModelFile(p)
    tiny = (m, ModelConfig.from_header(m.header))
    want = [solo(tiny, prompt, rel=True)
            for prompt in (SHARED_A, OTHER, SHARED_B)]
    model = HipTransformer.from_file(m, tiny[1], n_slots=3, kv_pages=16,
                                     page_size=P)
    eng = BatchEngine(model)
    a = eng.submit(SHARED_A, MAX_TOKENS)
    c = eng.submit(OTHER, MAX_TOKENS)
    eng.run()
    b = eng.submit(SHARED_B, MAX_TOKENS)
    eng.step()
    assert [pos for s, pos in eng.last_step_rows if s is b] == list(range(8, 13))
    eng.run()
    assert [a.tokens, c.tokens, b.tokens] == want
    assert [s.stats.cached_tokens for s in (a, c, b)] == [0, 0, 8]
    _pool_settled(eng)
    assert model._row_graphs  # the all-decode steps replayed captured graphs
