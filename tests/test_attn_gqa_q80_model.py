"""The drive of tests/test_attn_gqa_model.py on a Q80 cache at option level 2
against CpuTransformer with the same kv_dtype (the same K/V round trip)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd.models.cpu_model import CpuTransformer
from test_attn_chunk_model import case  # noqa: F401  (model file, config)
from test_attn_gqa_model import DECODE, SLOTS, TOKENS


@pytest.mark.parametrize("kw", [{}, dict(kv_pages=8, page_size=32)],
                         ids=["unpaged", "paged"])
def test_gqa_attn_q80_decode_rows_match_cpu(case, kw):
    from dllama_amd.models.hip_model import HipTransformer
    m, cfg, _, tol = case
    want = [CpuTransformer(m, cfg, kv_dtype="q80").forward(
        torch.tensor(t), torch.arange(len(t)))[-DECODE:] for t in TOKENS]
    hip = HipTransformer.from_file(m, cfg, n_slots=2, kv_dtype="q80", **kw)
    hip.set_gqa_attn(True, q80=True)
    for slot, pages in enumerate([[5, 2], [7, 3]] if kw else []):
        hip.set_slot_pages(slot, pages)
    for toks, slot in zip(TOKENS, SLOTS):
        for a in range(0, len(toks) - DECODE, 32):
            at = list(range(a, min(a + 32, len(toks) - DECODE)))
            hip.forward_rows([toks[p] for p in at], [slot] * len(at), at)
    for i in range(DECODE):
        at = [len(t) - DECODE + i for t in TOKENS]
        got = hip.forward_rows([t[p] for t, p in zip(TOKENS, at)],
                               list(SLOTS), at).cpu()
        assert hip.attn_splits == 8 and hip._gqa_step()
        w = torch.stack([w[i] for w in want])
        err = (got - w).abs().max().item() / (w.abs().max().item() + 1e-9)
        print(f"step {i}: rel err {err:.3e} (tolerance {tol})")
        assert err < tol and torch.equal(got.argmax(-1), w.argmax(-1))


def test_gqa_attn_env_level_2(case, monkeypatch):
    from dllama_amd.models.hip_model import HipTransformer
    monkeypatch.setenv("DLLAMA_ATTN_GQA", "2")
    hip = HipTransformer.from_file(*case[:2], n_slots=2, kv_dtype="q80")
    assert hip.gqa_attn and hip.gqa_attn_q80
