"""q40_gemm_tile / q40_gemm_tile_resid against the exact integer oracle
(reference.q40_q80_exact), every element within reference.q40_q80_bound: the
oracle, tolerance and input families of test_gemm_stream, 128 live input rows.
Outputs carry a guard row that must stay 7.0."""

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
# less than a weight tile and one block / partial last tile, 5 blocks / 9
# blocks / 131 blocks: odd chunk trip counts and a partial last chunk
SHAPES = [(8, 32), (69, 160), (160, 288), (64, 4192)]
# both sides of every 16- and 32-row activation sub-tile edge that matters
BATCHES = (1, 31, 33, 64, 65, 96, 127, 128)
# from d = 6144 a workgroup takes 32 weight rows (two row tiles, two column
# tiles per wave): a partial last tile with one block, and with 9 blocks
SHAPES_RT2 = [(6150, 32), (6160, 288)]
CASES = [(d, n, b) for d, n in SHAPES for b in BATCHES] + [
    (d, n, b) for d, n in SHAPES_RT2 for b in (64, 65, 128)]


@pytest.fixture(scope="module")
def k():
    from dllama_amd.ops import hip_ops
    return hip_ops()


@functools.lru_cache(maxsize=None)
def _case(family, d, n):
    """(qs, sc, xq, xs, xbs) on the device, 128 live input rows, and the
    oracle's (y, A). Built once per key; nothing writes to it."""
    qs, sc, xq, xs, xbs = adversarial_q40_q80(d, n, 128, 11)
    if family == "natural":
        qs, sc = natural_q40_planes(d, n, 12)
        g = torch.Generator().manual_seed(13)
        xq, xs, xbs = R.q80_quantize(torch.randn(128, n, generator=g) * 0.5)
    y, A = R.q40_q80_exact(qs, sc, xq, xs)
    return tuple(t.to(DEV).contiguous() for t in (qs, sc, xq, xs, xbs)), y, A


def _check(got, want, tol, what):
    err = (got.detach().cpu().double() - want).abs()
    assert (err <= tol).all(), (what, (err / tol).max().item())


@pytest.mark.parametrize("d,n,batch", CASES)
@pytest.mark.parametrize("family", FAMILIES)
def test_q40_gemm_tile(k, family, d, n, batch):
    (qs, sc, xq, xs, xbs), y, A = _case(family, d, n)
    tol = R.q40_q80_bound(n // 32, A[:batch])
    # rows past `batch` of the inputs are live data; then exactly `batch` rows
    for acts in ((xq, xs, xbs), tuple(t[:batch].clone() for t in (xq, xs, xbs))):
        out = torch.full((batch + 1, d), FILL, device=DEV)
        k.q40_gemm_tile(qs, sc, *acts, out, batch)
        _check(out[:batch], y[:batch], tol, (family, d, n, batch))
        assert (out[batch] == FILL).all(), "write past row `batch`"


@pytest.mark.parametrize("batch", (33, 128))
@pytest.mark.parametrize("d,n", [(69, 160), (64, 4192)] + SHAPES_RT2)
@pytest.mark.parametrize("family", FAMILIES)
def test_q40_gemm_tile_resid(k, family, d, n, batch):
    ins, y, A = _case(family, d, n)
    g = torch.Generator().manual_seed(14)
    x0 = torch.randn(batch + 1, d, generator=g).to(DEV)
    x0[batch] = FILL
    x = x0.clone()
    ssq = torch.zeros(batch + 1, 16 * 32, device=DEV)
    k.q40_gemm_tile_resid(*ins, x, ssq, batch)
    want = x0[:batch].cpu().double() + y[:batch]
    # one more f32 add, x0 + y_kernel: u * |x0 + y|
    _check(x[:batch], want, R.q40_q80_bound(n // 32, A[:batch]) + U * want.abs(),
           (family, d, n, batch))
    total = ssq.cpu().double().reshape(-1, 16, 32)[:, :, 0].sum(-1)
    assert torch.allclose(total[:batch], (want ** 2).sum(-1), rtol=1e-4)
    assert (x[batch] == FILL).all() and (ssq[batch] == 0).all()


@pytest.mark.parametrize("d,n", [(69, 160), (64, 4192), (6160, 288)])
def test_row_independence(k, d, n):
    """Rows 3 and 40 have the same bits at batch 41, 96 and 128: columns never
    mix, and no part of a row's summation order comes from `batch`."""
    ins = _case("adversarial", d, n)[0]
    rows = []
    for batch in (41, 96, 128):
        out = torch.zeros(batch, d, device=DEV)
        k.q40_gemm_tile(*ins, out, batch)
        rows.append(out[[3, 40]].clone())
    assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])
