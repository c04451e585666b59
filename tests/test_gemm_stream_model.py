"""HipTransformer with set_stream_gemm(True): prompt chunks and row steps
against the CPU model, with the models, comparison and tolerance of
test_rows_model; graph replays against eager steps; the switch back."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd.models.cpu_model import CpuTransformer
from test_rows_model import TOL, _hip, _rel_err, models  # noqa: F401

ARCHS = ("llama", "qwen3moe")


def _tokens(n=32):
    return torch.randint(0, 256, (n,), generator=torch.Generator().manual_seed(5))


def _stream(models, arch, **kw):  # noqa: F811
    model = _hip(models, arch, **kw)
    model.set_stream_gemm(True)
    assert model.stream_gemm and model.stream_gemm_min_rows == 8
    return model


@pytest.fixture(scope="module")
def want(models):  # noqa: F811
    """Per arch the CPU logits of the 32-token prompt and of each of its
    first 8 tokens alone at position 0. Computed once, never written."""
    out = {}
    for arch in ARCHS:
        m, cfg = models[arch]
        t = _tokens()
        out[arch] = (CpuTransformer(m, cfg).forward(t, torch.arange(32)),
                     [CpuTransformer(m, cfg).forward(t[i:i + 1], torch.arange(1))[0]
                      for i in range(8)])
    return out


@pytest.mark.parametrize("rows", (9, 32))
@pytest.mark.parametrize("arch", ARCHS)
def test_chunk_matches_cpu(models, want, arch, rows):  # noqa: F811
    got = _stream(models, arch).forward(_tokens()[:rows], torch.arange(rows)).cpu()
    for i in range(rows):
        err = _rel_err(got[i], want[arch][0][i])
        assert err < TOL[arch], (arch, i, err)


@pytest.mark.parametrize("arch", ARCHS)
def test_row_step_matches_cpu(models, want, arch):  # noqa: F811
    got = _stream(models, arch, n_slots=8).forward_rows(
        _tokens()[:8].tolist(), [5, 2, 7, 0, 1, 6, 3, 4], [0] * 8).cpu()
    for i in range(8):
        err = _rel_err(got[i], want[arch][1][i])
        assert err < TOL[arch], (arch, i, err)


@pytest.mark.parametrize("arch", ARCHS)
def test_row_graph_equals_eager(models, arch):  # noqa: F811
    """Two replays of the captured 8-row step, same bits as eager steps. (At
    dim 64 the residual fold's 4 workgroups each own an ssq slot, so the
    float atomics have no order to differ in.)"""
    eager = _stream(models, arch, n_slots=8)
    eager.row_graphs = False
    graphed = _stream(models, arch, n_slots=8)
    t = _tokens()
    for pos in range(3):
        step = (t[8 * pos:8 * pos + 8].tolist(), list(range(8)), [pos] * 8)
        a = eager.forward_rows(*step).cpu().clone()
        b = graphed.forward_rows(*step).cpu().clone()
        assert torch.equal(a, b), (arch, pos)
    assert not eager._row_graphs and list(graphed._row_graphs) == [8]


@pytest.mark.parametrize("arch", ARCHS)
def test_switch_off_restores(models, arch):  # noqa: F811
    model, t = _hip(models, arch), _tokens()[:9]
    assert model.stream_gemm is False
    off = model.forward(t, torch.arange(9)).cpu().clone()
    model.set_stream_gemm(True)
    model.forward(t, torch.arange(9))
    model.set_stream_gemm(False)
    assert torch.equal(model.forward(t, torch.arange(9)).cpu(), off)
