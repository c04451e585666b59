"""q40_gemm_stream / q40_gemm_stream_resid against the exact integer oracle
(reference.q40_q80_exact), every element within reference.q40_q80_bound.
Inputs are asymmetric and random, so an operand or output transpose of the
MFMA fragments cannot hide. Outputs carry a guard row that must stay 7.0."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd.ops import reference as R
from dllama_amd.utils.testing import adversarial_q40_q80, natural_q40_planes

DEV = "cuda"
U = 2.0 ** -24
FILL = 7.0
FAMILIES = ("natural", "adversarial")
# less than a row tile and one block / partial last tile, 5 blocks / 9 blocks
# / 131 blocks: ring and chunk trips and a partial last chunk
SHAPES = [(8, 32), (69, 160), (160, 288), (64, 4192)]
BATCHES = (1, 5, 8, 9, 16, 17, 32)


@pytest.fixture(scope="module")
def k():
    from dllama_amd.ops import hip_ops
    return hip_ops()


@functools.lru_cache(maxsize=None)
def _case(family, d, n):
    """(qs, sc, xq, xs, xbs) on the device, 32 live input rows, and the
    oracle's (y, A). Built once per key; nothing writes to it."""
    qs, sc, xq, xs, xbs = adversarial_q40_q80(d, n, 32, 11)
    if family == "natural":
        qs, sc = natural_q40_planes(d, n, 12)
        g = torch.Generator().manual_seed(13)
        xq, xs, xbs = R.q80_quantize(torch.randn(32, n, generator=g) * 0.5)
    y, A = R.q40_q80_exact(qs, sc, xq, xs)
    return tuple(t.to(DEV).contiguous() for t in (qs, sc, xq, xs, xbs)), y, A


def _check(got, want, tol, what):
    err = (got.detach().cpu().double() - want).abs()
    assert (err <= tol).all(), (what, (err / tol).max().item())


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("d,n", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_q40_gemm_stream(k, family, d, n, batch):
    (qs, sc, xq, xs, xbs), y, A = _case(family, d, n)
    tol = R.q40_q80_bound(n // 32, A[:batch])
    # rows past `batch` of the inputs are live data; then exactly `batch` rows
    for acts in ((xq, xs, xbs), tuple(t[:batch].clone() for t in (xq, xs, xbs))):
        out = torch.full((batch + 1, d), FILL, device=DEV)
        k.q40_gemm_stream(qs, sc, *acts, out, batch)
        _check(out[:batch], y[:batch], tol, (family, d, n, batch))
        assert (out[batch] == FILL).all(), "write past row `batch`"


@pytest.mark.parametrize("batch", (8, 32))
@pytest.mark.parametrize("d,n", [(69, 160), (64, 4192)])
@pytest.mark.parametrize("family", FAMILIES)
def test_q40_gemm_stream_resid(k, family, d, n, batch):
    ins, y, A = _case(family, d, n)
    g = torch.Generator().manual_seed(14)
    x0 = torch.randn(batch + 1, d, generator=g).to(DEV)
    x0[batch] = FILL
    x = x0.clone()
    ssq = torch.zeros(batch + 1, 16 * 32, device=DEV)
    k.q40_gemm_stream_resid(*ins, x, ssq, batch)
    want = x0[:batch].cpu().double() + y[:batch]
    # one more f32 add, x0 + y_kernel: u * |x0 + y|
    _check(x[:batch], want, R.q40_q80_bound(n // 32, A[:batch]) + U * want.abs(),
           (family, d, n, batch))
    total = ssq.cpu().double().reshape(-1, 16, 32)[:, :, 0].sum(-1)
    assert torch.allclose(total[:batch], (want ** 2).sum(-1), rtol=1e-4)
    assert (x[batch] == FILL).all() and (ssq[batch] == 0).all()


@pytest.mark.parametrize("d,n", [(69, 160), (64, 4192)])
def test_row_independence(k, d, n):
    """Row 3 has the same bits at batch 5, 16 and 32: columns never mix, and
    the work split comes from (d, n) alone, so this holds across NT too."""
    ins = _case("adversarial", d, n)[0]
    rows = []
    for batch in (5, 16, 32):
        out = torch.zeros(batch, d, device=DEV)
        k.q40_gemm_stream(*ins, out, batch)
        rows.append(out[3].clone())
    assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])
