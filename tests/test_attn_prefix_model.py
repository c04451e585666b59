"""The shared-prefix attention through forward_rows on a tiny paged model:
three slots mapped to the same two leading pages (32 tokens) plus pages of
their own, and one unrelated slot. With set_prefix_attn on, the logits of a
decode step stay within the tolerance of tests/test_attn_gqa_model.py (0.02
llama, 0.03 qwen3) of the same model with it off, and a greedy decode through
the captured row graph gives the same tokens, while one slot leaves the
group and another joins it under the replayed graph."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_attn_chunk_model import case  # noqa: F401  (model file, config)

P = 16
SHARED = [11, 4]
OWN = {0: 7, 1: 2, 2: 9, 4: 13}        # slot -> its page behind the prefix
PROMPT = [(7 * i + 3) % 256 for i in range(32)]
OTHER = [(11 * i + 5) % 256 for i in range(40)]
TAILS = {0: [17, 99, 3], 1: [], 2: [250, 1, 64, 8, 120]}  # own prompt tokens


def drive(m, cfg, kv_dtype, on):
    """(logits of the first decode step, tokens of 6 greedy steps, model)."""
    from dllama_amd.models.hip_model import HipTransformer
    hip = HipTransformer.from_file(m, cfg, n_slots=5, kv_pages=16, page_size=P,
                                   kv_dtype=kv_dtype)
    hip.set_prefix_attn(on, q80=True)
    hip.set_chunk_attn(True, q80=True)  # the prompt chunks take k_attn_chunk
    hip.prefix_min_tokens, hip.prefix_min_rows = 2 * P, 2
    hip.set_slot_pages(0, SHARED)
    hip.forward_rows(PROMPT, [0] * 32, list(range(32)))
    hip.set_slot_pages(3, [5, 12, 1])
    for a in (0, 32):
        hip.forward_rows(OTHER[a: a + 32], [3] * len(OTHER[a: a + 32]),
                         list(range(a, min(a + 32, 40))))
    for slot, page in OWN.items():
        if slot:
            hip.set_slot_pages(slot, SHARED)
        hip.set_slot_pages(slot, [page], first=2)
    for slot, tail in TAILS.items():
        if tail:
            hip.forward_rows(tail, [slot] * len(tail),
                             list(range(32, 32 + len(tail))))
    slots = [0, 1, 2, 3]
    at = [32 + len(TAILS[0]), 32, 32 + len(TAILS[2]), 40]
    tokens = [5, 200, 77, 31]
    logits = hip.forward_rows(tokens, slots, at).cpu().clone()
    picked = []
    for step in range(6):
        if step == 3:  # slot 2 leaves, slot 4 joins at its first own token
            hip.clear_slot(2)
            slots[2], at[2], tokens[2] = 4, 32, 142
        tokens = hip.forward_rows_sample(tokens, slots, at, [0.5] * 4,
                                         [0.0] * 4, [0.9] * 4)
        at = [p + 1 for p in at]
        picked.append(list(tokens))
    return logits, picked, hip


@pytest.mark.parametrize("kv_dtype", ["f16", "q80"])
def test_prefix_attn_rows_match_option_off(case, kv_dtype):
    m, cfg, _, tol = case
    want, want_tokens, off = drive(m, cfg, kv_dtype, False)
    got, got_tokens, hip = drive(m, cfg, kv_dtype, True)
    assert not off._prefix_step() and off.pre_ml is None
    # every row step took the three launches; the last ones found one group
    # of three behind the 32 shared tokens, slot 4 in slot 2's place
    assert hip._prefix_step() and hip.attn_splits == 8
    pre, groups, members, n = hip._pre_dev
    assert n == 1 and groups[0] == [0, 3] and members[:3] == [0, 1, 2]
    assert pre[:4] == [[0, 2 * P]] * 3 + [[-1, 0]]
    assert 4 in hip._row_graphs  # the decode steps replayed one graph
    err = (got - want).abs().max().item() / (want.abs().max().item() + 1e-9)
    print(f"{kv_dtype}: rel err on against off {err:.3e} (tolerance {tol})")
    assert err < tol
    assert torch.equal(got.argmax(-1), want.argmax(-1))
    assert got_tokens == want_tokens
