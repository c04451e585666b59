"""The chunk attention through the public path: a 70-token prompt (two full
32-row chunks and a ragged one) prefilled with set_chunk_attn(True) matches
CpuTransformer within the tolerances of tests/test_hip_model.py (0.02 llama,
0.03 qwen3), through forward and through forward_rows into slot 1; a Q80
cache with the option on computes what it computes with it off."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd import model_file as mf
from dllama_amd.models.config import ModelConfig
from dllama_amd.models.cpu_model import CpuTransformer
from dllama_amd.utils.testing import make_tiny_llama

PROMPT = [(7 * i + 3) % 256 for i in range(70)]
CHUNKS = [(0, 32), (32, 64), (64, 70)]


@pytest.fixture(scope="module", params=[("llama", 0.02), ("qwen3", 0.03)],
                ids=["llama", "qwen3"])
def case(request, tmp_path_factory):
    """(model file, config, CPU logits of the last chunk, tolerance)."""
    arch, tol = request.param
    p = str(tmp_path_factory.mktemp("m") / f"{arch}.m")
    if arch == "llama":
        make_tiny_llama(p, vocab_size=256)
    else:  # the tiny qwen3 of utils.testing with room for the prompt
        h = mf.LlmHeader(arch_type=mf.ARCH_QWEN3, dim=64, hidden_dim=96,
                         n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64,
                         vocab_size=256, seq_len=128, rope_theta=10000,
                         norm_epsilon=1e-6)
        h.finalize()
        mf.write_synthetic_model(p, h, seed=9)
    m = mf.ModelFile(p)
    cfg = ModelConfig.from_header(m.header)
    cpu = CpuTransformer(m, cfg)
    for a, b in CHUNKS:
        want = cpu.forward(torch.tensor(PROMPT[a:b]), torch.arange(a, b))
    return m, cfg, want.clone(), tol


def prefill(m, cfg, slot=None, chunk=True, **kw):
    from dllama_amd.models.hip_model import HipTransformer
    hip = HipTransformer.from_file(m, cfg, **kw)
    hip.set_chunk_attn(chunk)
    for a, b in CHUNKS:
        if slot is None:
            got = hip.forward(torch.tensor(PROMPT[a:b]), torch.arange(a, b))
        else:
            got = hip.forward_rows(PROMPT[a:b], [slot] * (b - a),
                                   list(range(a, b)))
    return hip, got.cpu().clone()


@pytest.mark.parametrize("slot", [None, 1], ids=["forward", "forward_rows"])
def test_chunk_attn_prefill_matches_cpu(case, slot):
    m, cfg, want, tol = case
    hip, got = prefill(m, cfg, slot, n_slots=1 if slot is None else 2)
    # the option routes chunk steps to the chunk binding, and only these
    assert hip._chunk_step(32, hip.seq_addr) == ()
    assert hip._chunk_step(7, hip.seq_addr) is None
    err = (got - want).abs().max().item() / (want.abs().max().item() + 1e-9)
    print(f"rel err {err:.3e} (tolerance {tol})")
    assert err < tol
    assert torch.equal(got.argmax(-1), want.argmax(-1))


def test_chunk_attn_q80_cache_falls_back(case):
    m, cfg, _, _ = case
    on, got = prefill(m, cfg, kv_dtype="q80")
    assert on._chunk_step(32, on.seq_addr) is None
    assert torch.equal(got, prefill(m, cfg, chunk=False, kv_dtype="q80")[1])
