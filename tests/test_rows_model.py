"""HipTransformer.forward_rows: several sequences in their own KV slots,
stepped together in ragged steps, against the CPU oracle running each
sequence alone. Teacher-forced (fixed token lists), so one differing token
cannot cascade."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd import model_file as mf
from dllama_amd.models.config import ModelConfig
from dllama_amd.models.cpu_model import CpuTransformer
from dllama_amd.utils.testing import make_tiny_llama, make_tiny_qwen3

# prompts of 5, 1 and 9 tokens, then 4 forced decode tokens each. Chosen on
# the CPU oracle so every row's top-1/top-2 gap is above twice the tolerance
# (asserted in the oracle fixture): within the tolerance the argmax is then
# decided.
PROMPT_LENS = (5, 1, 9)
TOKENS = {
    "llama": [[61, 152, 140, 34, 235, 155, 122, 161, 149],
              [17, 156, 4, 215, 67],
              [60, 50, 215, 141, 122, 164, 221, 60, 238, 134, 190, 4, 172]],
    "qwen3": [[199, 41, 246, 152, 11, 8, 211, 222, 69],
              [236, 236, 110, 102, 206],
              [114, 225, 94, 25, 127, 56, 67, 248, 173, 112, 161, 219, 214]],
    "qwen3moe": [[147, 137, 150, 150, 60, 235, 238, 8, 72],
                 [156, 42, 147, 146, 55],
                 [163, 147, 73, 32, 17, 124, 219, 164, 124, 23, 89, 205, 230]],
}
TOL = {"llama": 0.02, "qwen3": 0.03, "qwen3moe": 0.03}
SLOT_OF = (2, 0, 3)  # sequence -> slot, not in row order; n_slots=4
# (sequence, rows) per step: prompt chunks and decode rows share steps, and
# the last four steps are all-decode (the captured row graphs)
SCHEDULE = [
    [(0, 3), (2, 4), (1, 1)],
    [(1, 1), (0, 2), (2, 3)],
    [(1, 1), (0, 1), (2, 2)],
    [(1, 1), (0, 1), (2, 1)],
    [(1, 1), (0, 1), (2, 1)],
    [(0, 1), (2, 1)],
    [(2, 1)],
]


def _rel_err(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-9)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("rows")
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
    """Per arch: the CPU logits of every sequence run alone. Computed once,
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


def _drive(model, arch, schedule=SCHEDULE, slot_of=SLOT_OF):
    """Step TOKENS[arch] through forward_rows along the schedule; returns
    per sequence the logits rows in position order."""
    seqs = TOKENS[arch]
    cursor = [0] * len(seqs)
    got = [[] for _ in seqs]
    for step in schedule:
        tokens, slots, positions, owner = [], [], [], []
        for s, n in step:
            for _ in range(n):
                tokens.append(seqs[s][cursor[s]])
                slots.append(slot_of[s])
                positions.append(cursor[s])
                owner.append(s)
                cursor[s] += 1
        logits = model.forward_rows(tokens, slots, positions).cpu()
        for b, s in enumerate(owner):
            got[s].append(logits[b].clone())
    assert cursor == [len(t) for t in seqs]
    return [torch.stack(g) for g in got]


def test_schedule_shape():
    """The schedule is what the docstrings say: prompts of 5, 1, 9 and four
    decode rows each, with mixed steps."""
    fed = [sum(n for step in SCHEDULE for s, n in step if s == i)
           for i in range(3)]
    assert fed == [p + 4 for p in PROMPT_LENS]
    assert all(len(TOKENS[a][i]) == fed[i] for a in TOKENS for i in range(3))


@pytest.mark.parametrize("arch", list(TOKENS))
def test_three_sequences_match_cpu(models, oracle, arch):
    hip = _hip(models, arch, n_slots=4)
    got = _drive(hip, arch)
    for s, (g, want) in enumerate(zip(got, oracle[arch])):
        for i in range(len(want)):
            err = _rel_err(g[i], want[i])
            print(f"{arch} seq {s} row {i}: rel err {err:.5f}")
            assert err < TOL[arch], (arch, s, i, err)
        assert torch.equal(g.argmax(-1), want.argmax(-1)), (arch, s)
    assert hip._row_graphs  # the all-decode steps replayed captured graphs


@pytest.mark.parametrize("arch", list(TOKENS))
def test_composition_invariance(models, arch):
    """Sequence 2 stepped alone, one row per step, and as row 2 of four:
    same math, another launch shape."""
    alone = _hip(models, arch, n_slots=4)
    toks = TOKENS[arch][2]
    want = torch.stack([alone.forward_rows([t], [1], [i]).cpu()[0].clone()
                        for i, t in enumerate(toks)])
    mixed = _hip(models, arch, n_slots=4)
    others = TOKENS[arch][0] + TOKENS[arch][1]
    got = []
    for i, t in enumerate(toks):
        o = others[i % len(others)]
        logits = mixed.forward_rows([o, o + 1, t, o + 2], [0, 2, 1, 3],
                                    [i, i, i, i]).cpu()
        got.append(logits[2].clone())
    err = _rel_err(torch.stack(got), want)
    print(f"{arch}: alone vs row 2 of 4 rel err {err:.2e}")
    assert err < 1e-4, err


def test_slot0_matches_forward(models):
    toks = TOKENS["llama"][2]
    plain = _hip(models, "llama")
    rows = _hip(models, "llama", n_slots=4)
    n = 9
    want = [plain.forward(torch.tensor(toks[:n]), torch.arange(n)).cpu().clone()]
    got = [rows.forward_rows(toks[:n], [0] * n, list(range(n))).cpu().clone()]
    for i in range(n, len(toks)):
        want.append(plain.forward(torch.tensor([toks[i]]),
                                  torch.tensor([i])).cpu().clone())
        got.append(rows.forward_rows([toks[i]], [0], [i]).cpu().clone())
    err = _rel_err(torch.cat(got), torch.cat(want))
    print(f"slot 0 forward_rows vs forward: rel err {err:.2e}")
    assert err < 0.01, err


@pytest.mark.parametrize("arch", list(TOKENS))
def test_row_graph_matches_eager(models, arch):
    """Four replays of the captured 3-row step against eager steps. After
    the first, the graphed model's table is only ever moved by the graph's
    own rows_advance."""
    eager = _hip(models, arch, n_slots=4)
    eager.row_graphs = False
    graphed = _hip(models, arch, n_slots=4)
    prefill = [[(0, 5), (1, 1), (2, 9)]]
    decode = [[(1, 1), (0, 1), (2, 1)]] * 4
    want = _drive(eager, arch, prefill + decode)
    copies = []
    graphed._rows_buffers()
    stage = graphed._stage_rows

    def counting_stage(*a, **kw):
        before = list(graphed._rows_dev)
        out = stage(*a, **kw)
        copies.append(before[: out[0]] != out[1])  # the table was sent
        return out

    graphed._stage_rows = counting_stage
    got = _drive(graphed, arch, prefill + decode)
    assert not eager._row_graphs and list(graphed._row_graphs) == [3]
    assert copies == [True, True, False, False, False]
    for s in range(3):
        err = _rel_err(got[s], want[s])
        print(f"{arch} seq {s}: graph vs eager rel err {err:.2e}")
        assert err < 1e-5, (arch, s, err)
    assert graphed.rows[:3, 1].tolist() == [5, 9, 13]


def test_n_slots_leaves_forward_alone(models):
    toks = torch.tensor(TOKENS["llama"][2])
    one = _hip(models, "llama")
    four = _hip(models, "llama", n_slots=4)
    assert four.k_cache[0].shape[0] == 4 * one.k_cache[0].shape[0]
    a = one.forward(toks[:9], torch.arange(9)).cpu().clone()
    b = four.forward(toks[:9], torch.arange(9)).cpu().clone()
    assert torch.equal(a, b)
    a = one.forward(toks[9:10], torch.tensor([9])).cpu().clone()
    b = four.forward(toks[9:10], torch.tensor([9])).cpu().clone()
    assert torch.equal(a, b)


@pytest.mark.parametrize("arch", ["llama", "qwen3moe"])
def test_tp_path_rows(models, arch):
    plain = _hip(models, arch, n_slots=4)
    tp = _hip(models, arch, n_slots=4, force_sync=True)
    want = _drive(plain, arch)
    got = _drive(tp, arch)
    for s in range(3):
        err = _rel_err(got[s], want[s])
        print(f"{arch} seq {s}: TP path vs plain rel err {err:.4f}")
        assert err < 0.02, (arch, s, err)


@pytest.mark.parametrize("force_sync", [False, True])
def test_forward_rows_sample_greedy(models, force_sync):
    """Temperature 0: every row's token is its argmax, in an eager mixed
    step and in replayed all-decode steps."""
    hip = _hip(models, "llama", n_slots=4, force_sync=force_sync)
    seqs = TOKENS["llama"]
    steps = [([seqs[0][0], seqs[0][1], seqs[2][0], seqs[1][0]],
              [2, 2, 3, 0], [0, 1, 0, 0]),
             ([seqs[0][2], seqs[2][1], seqs[1][1]], [2, 3, 0], [2, 1, 1]),
             ([seqs[0][3], seqs[2][2], seqs[1][2]], [2, 3, 0], [3, 2, 2])]
    for tokens, slots, positions in steps:
        B = len(tokens)
        picked = hip.forward_rows_sample(tokens, slots, positions, [0.0] * B,
                                         [0.0] * B, [0.9] * B)
        assert picked == hip.rows_logits(B).argmax(-1).tolist()
    assert list(hip._row_graphs) == [3]


def test_forward_rows_validation(models):
    hip = _hip(models, "llama", n_slots=2)
    with pytest.raises(ValueError, match="slot"):
        hip.forward_rows([1], [2], [0])
    with pytest.raises(ValueError, match="seq_len"):
        hip.forward_rows([1], [0], [hip.cfg.seq_len])
    with pytest.raises(ValueError, match="two rows"):
        hip.forward_rows([1, 2], [1, 1], [3, 3])
    with pytest.raises(ValueError, match="n_batches"):
        hip.forward_rows([1] * 33, [0] * 33, list(range(33)))
