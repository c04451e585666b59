"""The paged and Q80 forms of the chunk attention through the public path:
the 70-token prompt of tests/test_attn_chunk_model.py prefilled into a paged
model with set_chunk_attn(True), and into a Q80 cache (unpaged and paged)
with set_chunk_attn(True, q80=True), matches CpuTransformer with the same
kv_dtype within the tolerances of tests/test_hip_model.py; a slot that shares
another's prefix pages computes that slot's logits bit for bit."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd.models.cpu_model import CpuTransformer
from test_attn_chunk_model import CHUNKS, PROMPT, case  # noqa: F401

PAGED = dict(n_slots=2, kv_pages=8, page_size=32)


def model(case, q80=False, **kw):
    from dllama_amd.models.hip_model import HipTransformer
    hip = HipTransformer.from_file(*case[:2], kv_dtype="q80" if q80 else None,
                                   **kw)
    hip.set_chunk_attn(True, q80=q80)
    return hip


def prefill_rows(hip, slot, chunks=CHUNKS):
    """Each chunk as a row step; a step takes the chunk path exactly when it
    has chunk_min_rows rows."""
    for a, b in chunks:
        got = hip.forward_rows(PROMPT[a:b], [slot] * (b - a), list(range(a, b)))
        assert (hip.row_addr.chunk is not None) == (b - a >= hip.chunk_min_rows)
    return got.cpu().clone()


def check_close(got, want, tol):
    err = (got - want).abs().max().item() / (want.abs().max().item() + 1e-9)
    print(f"rel err {err:.3e} (tolerance {tol})")
    assert err < tol and torch.equal(got.argmax(-1), want.argmax(-1))


def test_chunk_attn_paged_prefill_and_shared_prefix(case):
    hip = model(case, **PAGED)
    hip.set_slot_pages(0, [5, 2, 7])
    got = prefill_rows(hip, 0)
    check_close(got, case[2], case[3])
    # slot 1: slot 0's two full pages, a page of its own, the last chunk only
    hip.set_slot_pages(1, [5, 2, 3])
    assert torch.equal(prefill_rows(hip, 1, CHUNKS[2:]), got)
    hip.forward_rows([1], [0], [70])
    assert hip.row_addr.chunk is None


@pytest.mark.parametrize("kw", [{}, dict(n_slots=2), PAGED],
                         ids=["forward", "forward_rows", "paged"])
def test_chunk_attn_q80_prefill_matches_cpu(case, kw):
    cpu = CpuTransformer(*case[:2], kv_dtype="q80")
    for a, b in CHUNKS:
        want = cpu.forward(torch.tensor(PROMPT[a:b]), torch.arange(a, b))
    hip = model(case, q80=True, **kw)
    assert hip._chunk_step(32, hip.seq_addr) == ()
    if kw is PAGED:
        hip.set_slot_pages(1, [5, 2, 7])
    if kw:
        got = prefill_rows(hip, 1)
    else:
        for a, b in CHUNKS:
            got = hip.forward(torch.tensor(PROMPT[a:b]), torch.arange(a, b)).cpu()
    check_close(got, want, case[3])
