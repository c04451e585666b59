"""The GQA-packed decode attention through forward_rows: two slots prefilled
with prompts of unequal length, then 6 all-decode steps, against CpuTransformer
within the tolerances of tests/test_attn_chunk_model.py (0.02 llama, 0.03
qwen3); the wide tier and a Q80 cache keep their old launches."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd.models.cpu_model import CpuTransformer
from test_attn_chunk_model import case  # noqa: F401  (model file, config)

# teacher-forced: a 40- and a 9-token prompt, then 6 decode tokens each
TOKENS = [[(7 * i + 3) % 256 for i in range(46)],
          [(11 * i + 5) % 256 for i in range(15)]]
SLOTS = (1, 0)
DECODE = 6


@pytest.fixture(scope="module")
def want(case):
    """Per sequence the CPU logits of its decode positions, run alone."""
    m, cfg, _, _ = case
    return [CpuTransformer(m, cfg).forward(
        torch.tensor(t), torch.arange(len(t)))[-DECODE:].clone()
        for t in TOKENS]


def drive(m, cfg, gqa, wide=False, **kw):
    """Prefill both slots, then the decode steps: (model, logits per step)."""
    from dllama_amd.models.hip_model import HipTransformer
    hip = HipTransformer.from_file(m, cfg, n_slots=2, **kw)
    hip.set_gqa_attn(gqa)
    hip.set_wide_rows(wide)
    for toks, slot in zip(TOKENS, SLOTS):
        for a in range(0, len(toks) - DECODE, 32):
            b = min(a + 32, len(toks) - DECODE)
            hip.forward_rows(toks[a:b], [slot] * (b - a), list(range(a, b)))
    steps = []
    for i in range(DECODE):
        at = [len(t) - DECODE + i for t in TOKENS]
        steps.append(hip.forward_rows([t[p] for t, p in zip(TOKENS, at)],
                                      list(SLOTS), at).cpu().clone())
    return hip, steps


def test_gqa_attn_decode_rows_match_cpu(case, want):
    m, cfg, _, tol = case
    hip, steps = drive(m, cfg, True)
    # a row step at S = 8 takes the new binding
    assert hip.attn_splits == 8 and hip._gqa_step()
    for i, got in enumerate(steps):
        w = torch.stack([w[i] for w in want])
        err = (got - w).abs().max().item() / (w.abs().max().item() + 1e-9)
        print(f"step {i}: rel err {err:.3e} (tolerance {tol})")
        assert err < tol
        assert torch.equal(got.argmax(-1), w.argmax(-1))


def test_gqa_attn_leaves_wide_tier_and_q80_cache(case):
    m, cfg, _, _ = case
    hip, wide_on = drive(m, cfg, True, wide=True)
    assert hip.attn_splits == 1 and not hip._gqa_step()
    for a, b in zip(wide_on, drive(m, cfg, False, wide=True)[1]):
        assert torch.equal(a, b)
    hip, q80_on = drive(m, cfg, True, kv_dtype="q80")
    assert hip.attn_splits == 8 and not hip._gqa_step()
    for a, b in zip(q80_on, drive(m, cfg, False, kv_dtype="q80")[1]):
        assert torch.equal(a, b)
