"""BatchEngine over the CPU model: many sequences through ragged steps
generate what each generates alone (InferenceEngine.generate), whatever they
are batched with, whichever slot they land in."""

import pytest
import torch

from dllama_amd import model_file as mf
from dllama_amd.engine import BatchEngine, InferenceEngine
from dllama_amd.models.config import ModelConfig
from dllama_amd.models.cpu_model import CpuTransformer
from dllama_amd.tokenizer import Sampler
from dllama_amd.utils.testing import make_tiny_llama

VOCAB = 256
SEQ_LEN = 48
# chosen on the oracle: top-1/top-2 logit gap > GAP at every generated step
# of the greedy and of the seeded runs below (asserted in _solo)
PROMPTS = [[65, 253, 233, 137, 252], [39],
           [217, 42, 88, 136, 65, 31, 153, 236, 114]]
GAP = 1e-3
MAX_TOKENS = 4
# fills the context window but for four rows; same gap property
LONG_PROMPT = [83, 214, 128, 128, 163, 172, 224, 52, 139, 157, 239, 57, 3, 88,
               181, 247, 192, 231, 82, 210, 83, 10, 135, 38, 224, 66, 155, 201,
               40, 216, 98, 150, 76, 184, 181, 207, 121, 17, 205, 22, 133, 223,
               235, 11]


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("be") / "tiny.m")
    # dim 256: the logits of narrower random models are too flat for the gap
    make_tiny_llama(p, vocab_size=VOCAB, seq_len=SEQ_LEN, dim=256)
    m = mf.ModelFile(p)
    return m, ModelConfig.from_header(m.header)


def _sampler(temperature, seed):
    return Sampler(VOCAB, temperature, 0.9, seed)


class _GapModel:
    """A model proxy recording the top-1/top-2 gap of every logits row a
    token is sampled from (the last row of each forward)."""

    def __init__(self, model):
        self._m = model
        self.gaps = []

    def __getattr__(self, name):
        return getattr(self._m, name)

    def forward(self, tokens, positions):
        logits = self._m.forward(tokens, positions)
        top = torch.topk(logits[-1], 2).values
        self.gaps.append(float(top[0] - top[1]))
        return logits


_solo_cache = {}


def _solo(tiny, prompt, temperature, seed, max_tokens=MAX_TOKENS):
    """The prompt generated alone; computed once per case and shared."""
    key = (tuple(prompt), temperature, seed, max_tokens)
    if key not in _solo_cache:
        m, cfg = tiny
        model = _GapModel(CpuTransformer(m, cfg))
        eng = InferenceEngine(model, sampler=_sampler(temperature, seed))
        out, _ = eng.generate(prompt, max_tokens)
        assert min(model.gaps) > GAP, (prompt, model.gaps)
        _solo_cache[key] = out
    return list(_solo_cache[key])


@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_queueing_matches_solo(tiny, temperature):
    """Three prompts on two slots: one waits, every one generates what it
    generates alone, greedy and seeded."""
    m, cfg = tiny
    eng = BatchEngine(CpuTransformer(m, cfg, n_slots=2))
    seeds = [11, 12, 13]
    got = eng.generate_many(
        PROMPTS, MAX_TOKENS,
        samplers=[_sampler(temperature, s) for s in seeds])
    assert len(eng.free_slots) == 2 and eng.idle
    for prompt, seed, (tokens, stats) in zip(PROMPTS, seeds, got):
        assert tokens == _solo(tiny, prompt, temperature, seed)
        assert stats.prefill_tokens == len(prompt)
        assert stats.decode_tokens == len(tokens)


def test_scheduling(tiny):
    """No step exceeds n_batches rows, every running sequence gets exactly
    one decode row per step, and prompts longer than the room are chunked."""
    m, cfg = tiny
    eng = BatchEngine(CpuTransformer(m, cfg, n_slots=3), n_batches=4)
    seqs = [eng.submit(p, MAX_TOKENS) for p in PROMPTS]
    steps = 0
    while not eng.idle:
        eng._plan()  # admits waiting sequences; planning twice changes nothing
        decoding = [s for s in eng.running if not s.prefilling]
        eng.step()
        rows = eng.last_step_rows
        assert 1 <= len(rows) <= 4
        for s in decoding:
            assert sum(1 for r, _ in rows if r is s) == 1
        # decode rows come first
        assert [r for r, _ in rows[: len(decoding)]] == decoding
        steps += 1
    assert steps > MAX_TOKENS  # the 9-token prompt could not go in one step
    for prompt, s in zip(PROMPTS, seqs):
        assert s.done and s.tokens == _solo(tiny, prompt, 0.0, 12345)


def test_slot_reuse(tiny):
    """One slot: the second sequence runs over the first one's stale KV rows
    and still equals its solo run."""
    m, cfg = tiny
    eng = BatchEngine(CpuTransformer(m, cfg, n_slots=1))
    long_first = [PROMPTS[2], PROMPTS[0]]
    got = eng.generate_many(long_first, MAX_TOKENS)
    for prompt, (tokens, _) in zip(long_first, got):
        assert tokens == _solo(tiny, prompt, 0.0, 12345)


def test_stopping_is_per_sequence(tiny):
    m, cfg = tiny
    solo = [_solo(tiny, p, 0.0, 12345) for p in PROMPTS]
    eng = BatchEngine(CpuTransformer(m, cfg, n_slots=3))
    stop_tok = solo[0][2]
    cut = solo[0].index(stop_tok) + 1
    a = eng.submit(PROMPTS[0], MAX_TOKENS, stop_check=lambda t: t == stop_tok)
    b = eng.submit(PROMPTS[1], 2)
    seen = []
    c = eng.submit(PROMPTS[2], MAX_TOKENS, on_token=seen.append)
    eng.run()
    assert a.tokens == solo[0][:cut]      # its stop token, included
    assert b.tokens == solo[1][:2]        # its own max_tokens
    assert c.tokens == solo[2] == seen    # untouched by the others' ends


def test_context_end(tiny):
    """A sequence ends at the end of the context window as generate does,
    without disturbing its neighbour."""
    m, cfg = tiny
    prompt = LONG_PROMPT
    assert len(prompt) == SEQ_LEN - 4
    want = _solo(tiny, prompt, 0.0, 12345, max_tokens=50)
    assert len(want) < 50
    eng = BatchEngine(CpuTransformer(m, cfg, n_slots=2))
    got = eng.generate_many([prompt, PROMPTS[0]], 50)
    assert got[0][0] == want
    assert got[1][0][:MAX_TOKENS] == _solo(tiny, PROMPTS[0], 0.0, 12345)
    with pytest.raises(ValueError):
        eng.submit(list(range(SEQ_LEN + 1)), 4)


def test_forward_rows_validation(tiny):
    m, cfg = tiny
    model = CpuTransformer(m, cfg, n_slots=2, n_batches=4)
    model.forward_rows([1, 2], [0, 1], [0, 0])  # fine
    with pytest.raises(ValueError, match="slot"):
        model.forward_rows([1], [2], [0])
    with pytest.raises(ValueError, match="seq_len"):
        model.forward_rows([1], [0], [SEQ_LEN])
    with pytest.raises(ValueError, match="two rows"):
        model.forward_rows([1, 2], [1, 1], [3, 3])
    with pytest.raises(ValueError, match="n_batches"):
        model.forward_rows([1] * 5, [0] * 5, list(range(5)))


def test_forward_rows_matches_forward(tiny):
    """Rows of a sequence in slot 1, chunked unevenly and mixed with another
    slot's rows, give the logits of the plain forward."""
    m, cfg = tiny
    tokens = PROMPTS[2]
    want = CpuTransformer(m, cfg).forward(torch.tensor(tokens),
                                          torch.arange(len(tokens)))
    model = CpuTransformer(m, cfg, n_slots=3)
    a = model.forward_rows(tokens[:4] + [8], [1] * 4 + [2], [0, 1, 2, 3, 0])
    b = model.forward_rows([8] + tokens[4:], [0] + [1] * 5, [0, 4, 5, 6, 7, 8])
    got = torch.cat([a[:4], b[1:]])
    assert torch.allclose(got, want, atol=1e-6, rtol=1e-4)
