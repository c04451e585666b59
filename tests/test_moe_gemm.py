"""The expert-grouped MFMA GEMM of multi-row MoE steps: moe_group's routing
plan, q40_gemm_grouped in its plain and SwiGLU forms against the exact
integer oracle (reference.q40_q80_exact within q40_q80_bound, Q80 output
through q80_emit_check), and HipTransformer with set_moe_gemm(True) against
CpuTransformer.

Both input families of dllama_amd.utils.testing; every output buffer is
prefilled with 7.0 and carries one guard slot that must stay 7.0; the input
triple has live rows past the step's rows, which must not be reached."""

import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd import model_file as mf
from dllama_amd.models.config import ModelConfig
from dllama_amd.models.cpu_model import CpuTransformer
from dllama_amd.ops import reference as R
from dllama_amd.utils.testing import (adversarial_q40_q80, make_tiny_qwen3,
                                      natural_q40_planes)

DEV = "cuda"
FAMILIES = ("natural", "adversarial")
FILL = 7.0
E, KA, XROWS = 8, 2, 72  # the longest routing reads 64 input rows
# fixed router logits for NB = 5: top-2 per row, experts 4 and 6 never chosen
LOGITS5 = [[2.0, 1.0, 0.1, 0.3, -3.0, 0.2, -3.0, 0.0],
           [0.1, 2.0, 1.0, 0.3, -3.0, 0.2, -3.0, 0.0],
           [2.0, 0.1, 0.2, 1.0, -3.0, 0.3, -3.0, 0.0],
           [0.0, 0.1, 0.2, 0.3, -3.0, 2.0, -3.0, 1.0],
           [1.0, 0.1, 0.2, 0.3, -3.0, 0.0, -3.0, 2.0]]
ROUTINGS = {
    "top2_nb5": R.moe_gate(torch.tensor(LOGITS5), KA)[0].reshape(-1).tolist(),
    "same_two_nb32": [5, 2] * 32,          # two full tiles
    "nb1": [6, 1],
    # expert 3 gets 40 slots (two tiles, 32 + 8), not in slot order
    "one_expert_40": [3 if s % 6 else 7 - s % 5 for s in range(48)],
}
PLAN_PERM, PLAN_TILES, PLAN_INTS = 4, 516, 516 + 3 * 528


@pytest.fixture(scope="module")
def k():
    from dllama_amd.ops import hip_ops
    return hip_ops()


@functools.lru_cache(maxsize=None)
def _case(k, family, rows, n):
    """Stacked planes [E, rows, ..], an input triple of XROWS live rows, and
    the oracle per expert: y, A [E, XROWS, rows]. Shared, never written."""
    if family == "adversarial":
        qs, sc = adversarial_q40_q80(E * rows, n, 1, 11)[:2]
        xq, xs = adversarial_q40_q80(1, n, XROWS, 12)[2:4]
    else:
        qs, sc = natural_q40_planes(E * rows, n, 13)
        x = torch.randn(XROWS, n, generator=torch.Generator().manual_seed(14)) * 0.5
        xq, xs, _ = R.q80_quantize(x)
    ya = [R.q40_q80_exact(qs[e * rows:(e + 1) * rows], sc[e * rows:(e + 1) * rows], xq, xs)
          for e in range(E)]
    dev = (qs.reshape(E, rows, n // 2).to(DEV), sc.reshape(E, rows, n // 32).to(DEV),
           xq.to(DEV), xs.float().to(DEV))
    return dev, torch.stack([t[0] for t in ya]), torch.stack([t[1] for t in ya])


def _plan(k, experts):
    idx = torch.tensor(experts, dtype=torch.int32, device=DEV)
    plan = torch.full((PLAN_INTS + 1,), 7, dtype=torch.int32, device=DEV)
    k.moe_group(idx, plan, E)
    assert plan[PLAN_INTS] == 7
    return plan


def _slots(y, A, experts, k_slots):
    sel = [(e, s // k_slots) for s, e in enumerate(experts)]
    return (torch.stack([y[e, b] for e, b in sel]),
            torch.stack([A[e, b] for e, b in sel]))


@pytest.mark.parametrize("routing", list(ROUTINGS))
def test_moe_group_plan(k, routing):
    """perm is the slots by (expert, slot); the tiles cover it in order, one
    expert each, at most 32 slots, within the fixed bound of the grid."""
    experts = ROUTINGS[routing]
    S = len(experts)
    plan = _plan(k, experts).cpu().tolist()
    assert plan[PLAN_PERM:PLAN_PERM + S] == sorted(range(S), key=lambda s: (experts[s], s))
    want = []
    for e in sorted(set(experts)):
        first = sum(x < e for x in experts)
        cnt = experts.count(e)
        want += [[e, first + o, min(32, cnt - o)] for o in range(0, cnt, 32)]
    assert plan[0] == len(want) <= min(E, S) + S // 32
    assert [plan[PLAN_TILES + 3 * t:PLAN_TILES + 3 * t + 3]
            for t in range(len(want))] == want


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("k_slots", [KA, 1])
@pytest.mark.parametrize("routing", list(ROUTINGS))
@pytest.mark.parametrize("d,n", [(69, 32), (160, 288), (129, 4192)])
def test_q40_gemm_grouped(k, family, d, n, routing, k_slots):
    experts = ROUTINGS[routing]
    S = len(experts)
    (qs, sc, xq, xs), y, A = _case(k, family, d, n)
    assert xq[-(-S // k_slots):].ne(0).any()
    ys, As = _slots(y, A, experts, k_slots)
    out = torch.full((S + 1, d), FILL, device=DEV)
    k.q40_gemm_grouped(qs, sc, xq, xs, _plan(k, experts), S, k_slots, y=out)
    got = out[:S].cpu().double()
    assert torch.isfinite(got).all()
    err, tol = (got - ys).abs(), R.q40_q80_bound(n // 32, As)
    assert (err <= tol).all(), (err / tol.clamp_min(1e-300)).max().item()
    assert (out[S] == FILL).all()
    if routing == "same_two_nb32":
        # column independence: each slot alone (S = 1) gives the same bits
        for s in (0, 1, 33, 62, 63):
            xr = s // k_slots
            one = torch.full((2, d), FILL, device=DEV)
            k.q40_gemm_grouped(qs, sc, xq[xr:xr + 1], xs[xr:xr + 1],
                               _plan(k, experts[s:s + 1]), 1, 1, y=one)
            assert torch.equal(one[0], out[s]), s


def _act64(a, gelu):
    if gelu:
        return 0.5 * a * (1.0 + torch.tanh(0.797884560802865 * (a + 0.044715 * a ** 3)))
    return a * torch.sigmoid(a)


def _swiglu_truth(ya, Aa, yg, Ag, nb, gelu):
    """v = act(a) * g and its v_tol, as derived beside
    test_q40_gemv_grouped_swiglu: the error of a (at most bound_a) passes
    through act with slope at most 1.1 (|silu'| <= 1.0999) or 1.13
    (|gelu'| <= 1.129), the error of g (bound_g) is scaled by |act(a)|, and
    2^-21 * |v| covers expf / tanhf and the two products."""
    act = _act64(ya, gelu)
    v = act * yg
    slope = 1.13 if gelu else 1.1
    v_tol = (slope * R.q40_q80_bound(nb, Aa) * yg.abs()
             + R.q40_q80_bound(nb, Ag) * act.abs() + 2.0 ** -21 * v.abs())
    return v, v_tol


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("ff", [32, 96])
@pytest.mark.parametrize("routing", ["top2_nb5", "one_expert_40"])
def test_q40_gemm_grouped_swiglu(k, family, gelu, ff, routing):
    n = 288
    experts = ROUTINGS[routing]
    S = len(experts)
    (qs, sc, xq, xs), y, A = _case(k, family, 2 * ff, n)
    ys, As = _slots(y, A, experts, KA)
    v, v_tol = _swiglu_truth(ys[:, :ff], As[:, :ff], ys[:, ff:], As[:, ff:],
                             n // 32, gelu)
    out = (torch.full((S + 1, ff), 7, dtype=torch.int8, device=DEV),
           torch.full((S + 1, ff // 32), FILL, device=DEV),
           torch.full((S + 1, ff // 32), FILL, device=DEV))
    k.q40_gemm_grouped(qs, sc, xq, xs, _plan(k, experts), S, KA,
                       oq=out[0], os=out[1], obs=out[2], gelu=gelu)
    R.q80_emit_check(out[0][:S], out[1][:S], out[2][:S], v, v_tol)
    assert all((t[S] == 7).all() for t in out)


# ------------------------------------------------------------------- model

TOL = 0.03  # tests/test_rows_model.py, qwen3moe


def _rel_err(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-9)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("moe_gemm") / "moe.m")
    make_tiny_qwen3(p, moe=True)
    m = mf.ModelFile(p)
    cfg = ModelConfig.from_header(m.header)
    tokens = torch.randint(0, 256, (32,), generator=torch.Generator().manual_seed(5))
    return m, cfg, tokens, CpuTransformer(m, cfg).forward(tokens, torch.arange(32))


def _hip(tiny, **kw):
    from dllama_amd.models.hip_model import HipTransformer
    model = HipTransformer.from_file(tiny[0], tiny[1], **kw)
    model.set_moe_gemm(True)
    return model


@pytest.mark.parametrize("rows,force_sync", [(32, False), (9, False), (9, True)])
def test_chunk_matches_cpu(tiny, rows, force_sync):
    _, _, tokens, want = tiny
    got = _hip(tiny, force_sync=force_sync).forward(
        tokens[:rows], torch.arange(rows)).cpu()
    for i in range(rows):
        assert _rel_err(got[i], want[i]) < TOL, (i, _rel_err(got[i], want[i]))


def test_row_step_matches_cpu(tiny):
    m, cfg, tokens, _ = tiny
    got = _hip(tiny, n_slots=8).forward_rows(
        tokens[:8].tolist(), list(range(8)), [0] * 8).cpu()
    for i in range(8):
        want = CpuTransformer(m, cfg).forward(tokens[i:i + 1], torch.arange(1))[0]
        assert _rel_err(got[i], want) < TOL, (i, _rel_err(got[i], want))


def test_graph_replays_equal_eager(tiny):
    """A full chunk replays its captured graph; twice from the graph and once
    eager, the logits are the same bits: the path has no atomics."""
    model, tokens = _hip(tiny), tiny[2]
    runs = [model.forward(tokens, torch.arange(32)).cpu().clone() for _ in range(2)]
    assert ("prefill", False) in model.graphs.entries
    model.graphs.failed.add("prefill")  # the store's switch to eager steps
    runs.append(model.forward(tokens, torch.arange(32)).cpu().clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_launch_lists():
    """On, from moe_gemm_min_rows rows: moe_group and q40_gemm_grouped, no
    grouped GEMV. Below it, and with the option off: the parent's launches."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "tools"))
    import launch_trace as lt
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = lt.write_models(d)["qwen3moe64"]
        names = {}
        for sync in ("plain", "sync_q80"):
            model, kernels, content = lt._recorded_model(path, "qwen3moe64", sync, "none")
            assert model.moe_gemm is False and model.moe_gemm_min_rows > 3
            for on, B in ((False, 20), (True, 20), (True, 3)):
                model.moe_gemm = on
                kernels.trace = lt.Trace(content)
                model.forward_buffers(B)
                names[sync, on, B] = [c[0] for c in kernels.trace.calls]
    for sync in ("plain", "sync_q80"):
        on = names[sync, True, 20]
        assert on.count("moe_group") == 2 and on.count("q40_gemm_grouped") == 4
        assert "q40_gemv_grouped" not in on and "swiglu_q80" not in on
        assert len(on) == len(names[sync, False, 20])
        assert "q40_gemv_grouped" in names[sync, False, 20]
        assert "moe_group" not in names[sync, False, 20] + names[sync, True, 3]
