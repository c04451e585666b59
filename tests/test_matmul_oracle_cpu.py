"""The exact Q40xQ80 oracle (reference.q40_q80_exact), its derived bound and
q80_emit_check, checked on the CPU: the oracle against an independent
float64 dequantise-and-matmul, the bound against an f32 model of the GEMV
kernel, and the bound's teeth against seven mutants of that model, two of
which the suite's former rule (2 % of the largest output) accepts."""

import functools

import numpy as np
import pytest
import torch

from dllama_amd.ops import reference as R
from dllama_amd.utils.testing import adversarial_q40_q80, natural_q40_planes

FAMILIES = ("natural", "adversarial")

# every (d, n, rows) of tests/test_matmul_exact.py, rows = its largest batch
SHAPES = [
    (69, 32, 32), (72, 160, 32), (64, 4192, 32), (2049, 64, 1), (2050, 160, 1),
    (69, 160, 32), (2050, 64, 4), (256, 160, 1), (96, 160, 1), (256, 4192, 9),
    (512, 256, 1), (2050, 256, 1),
    (8, 32, 1), (129, 160, 20), (160, 288, 32),
    (69, 768, 2), (96, 2112, 2), (66, 160, 2), (64, 160, 1), (192, 4192, 1),
]


@functools.lru_cache(maxsize=None)
def _inputs(family, d, n, rows, seed=0):
    """(qs, sc, xq, xs, xbs, x) CPU tensors; x is the f32 activation the
    natural family quantised (None for the adversarial one)."""
    if family == "adversarial":
        return adversarial_q40_q80(d, n, rows, 1000 + seed) + (None,)
    qs, sc = natural_q40_planes(d, n, 2000 + seed)
    g = torch.Generator().manual_seed(3000 + seed)
    x = torch.randn(rows, n, generator=g) * 0.5
    xq, xs, xbs = R.q80_quantize(x)
    return qs, sc, xq, xs, xbs, x


def kernel_model(qs, sc, xq, xs, xbs, mutant=None):
    """f32 numpy model of k_q40_gemv: unsigned nibble dot minus 8*blocksum,
    f32 sw*sx, lane l folds block pairs l, l+64, .. in order, lane 0 the odd
    trailing block, xor-tree wave reduce. mul+add where the kernel has fmaf,
    so it rounds once more per block than the kernel does.

    mutant: None or one of MUTANTS, each a defect a kernel could have."""
    qs, xq = qs.numpy(), xq.numpy()
    d, nb = qs.shape[0], qs.shape[1] // 16
    rows = xq.shape[0]
    by = qs.reshape(d, nb, 16).astype(np.int64)
    nib = np.concatenate([by & 0xF, by >> 4], axis=-1)        # 0..15
    codes = xq.reshape(rows, nb, 32).astype(np.int64)
    bsum = xbs.numpy().astype(np.float32).copy()
    sw16 = sc.numpy().astype(np.float16).copy()
    sx = xs.numpy().astype(np.float32).copy()
    if mutant == "bsum_off_by_one":
        bsum[0, nb // 2] += 1.0
    elif mutant == "scale_low_bits":
        sw16 = (sw16.view(np.uint16) & np.uint16(0xFFFC)).view(np.float16)
    elif mutant == "xscale_prev_block":
        sx[:, 1:] = sx[:, :-1].copy()
    elif mutant == "elem31_low_nibble":
        nib[:, :, 31] = nib[:, :, 15]
    elif mutant == "minus127_as_plus":
        r, j, i = np.argwhere(codes == -127)[0]
        codes[r, j, i] = 127
    elif mutant == "abs_weight_scale":
        sw16 = np.abs(sw16)
    idot = np.einsum("djk,bjk->bdj", nib, codes)              # [rows, d, nb]
    integer = idot.astype(np.float32) - np.float32(8.0) * bsum[:, None, :]
    p = sw16.astype(np.float32)[None] * sx[:, None, :]        # f32, rounds once
    term = p * integer                                        # f32
    acc = np.zeros((rows, d, 64), np.float32)
    for jp in range(nb // 2):
        lane = jp % 64
        acc[:, :, lane] = acc[:, :, lane] + term[:, :, 2 * jp]
        acc[:, :, lane] = acc[:, :, lane] + term[:, :, 2 * jp + 1]
    if nb & 1 and mutant != "drop_odd_tail":
        acc[:, :, 0] = acc[:, :, 0] + term[:, :, nb - 1]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lanes ^ off]
    assert acc.dtype == np.float32
    return torch.from_numpy(acc[:, :, 0].copy())


MUTANTS = ("bsum_off_by_one", "scale_low_bits", "xscale_prev_block",
           "drop_odd_tail", "elem31_low_nibble", "minus127_as_plus",
           "abs_weight_scale")


def _worst_ratio(got, qs, sc, xq, xs):
    """max over outputs of |got - y| / bound (0/0 counts as 0)."""
    y, A = R.q40_q80_exact(qs, sc, xq, xs)
    nb = xs.shape[-1]
    err = (got.double() - y).abs()
    bound = R.q40_q80_bound(nb, A)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return ratio.max().item()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d,n,rows", [(72, 160, 4), (69, 32, 2), (64, 4192, 2)])
def test_oracle_matches_float64_dequant_matmul(family, d, n, rows):
    qs, sc, xq, xs, _, _ = _inputs(family, d, n, rows)
    y, A = R.q40_q80_exact(qs, sc, xq, xs)
    # the f32 dequant is exact (4-bit integer x 11-bit f16 significand), and
    # so are int8 x f32 and their products in float64: only the float64 sum
    # over n rounds
    w = R.q40_planes_dequant(qs, sc).double()
    x = (xq.reshape(rows, -1, 32).double() * xs.double().unsqueeze(-1)).reshape(rows, n)
    want = x @ w.t()
    assert y.dtype == A.dtype == torch.float64
    assert ((y - want).abs() <= 1e-12 * A).all(), \
        ((y - want).abs() / A.clamp_min(1e-300)).max().item()
    assert (A >= y.abs()).all()
    # a block range sums to the whole
    nb = n // 32
    parts = [R.q40_q80_exact(qs, sc, xq, xs, blocks=(j0, j1))
             for j0, j1 in ((0, nb // 2), (nb // 2, nb))]
    assert ((parts[0][0] + parts[1][0] - y).abs() <= 1e-12 * A).all()
    assert ((parts[0][1] + parts[1][1] - A).abs() <= 1e-12 * A).all()
    y0, A0 = R.q40_q80_exact(qs, sc, xq, xs, blocks=(1, 1))
    assert (y0 == 0).all() and (A0 == 0).all()


def test_oracle_by_hand():
    """One block, one row, written out: nibble layout and signs."""
    by = torch.arange(16, dtype=torch.uint8) | (torch.arange(15, -1, -1, dtype=torch.uint8) << 4)
    qs = by.reshape(1, 16)
    w = [j - 8 for j in range(16)] + [(15 - j) - 8 for j in range(16)]
    assert R.q40_unpack(qs).reshape(-1).tolist() == w
    codes = [((7 * i) % 255) - 127 for i in range(32)]
    xq = torch.tensor(codes, dtype=torch.int8).reshape(1, 32)
    sc = torch.tensor([[-0.25]], dtype=torch.float16)
    xs = torch.tensor([[0.5]])
    y, A = R.q40_q80_exact(qs, sc, xq, xs)
    dot = sum(a * b for a, b in zip(w, codes))
    assert y.item() == -0.125 * dot and A.item() == 0.125 * abs(dot)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d,n,rows", SHAPES)
def test_kernel_model_within_bound(family, d, n, rows):
    qs, sc, xq, xs, xbs, _ = _inputs(family, d, n, rows)
    got = kernel_model(qs, sc, xq, xs, xbs)
    ratio = _worst_ratio(got, qs, sc, xq, xs)
    print(f"model err/bound {family} d={d} n={n} rows={rows}: {ratio:.4f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("mutant", MUTANTS)
def test_bound_rejects_mutant(family, mutant):
    """n = 160: five blocks, so two block pairs and the odd trailing block."""
    d, n, rows = 72, 160, 4
    qs, sc, xq, xs, xbs, _ = _inputs(family, d, n, rows)
    if mutant == "abs_weight_scale":
        assert (sc < 0).any()
    if mutant == "scale_low_bits":
        assert (sc.view(torch.int16) & 3).ne(0).any()
    got = kernel_model(qs, sc, xq, xs, xbs, mutant)
    ratio = _worst_ratio(got, qs, sc, xq, xs)
    print(f"mutant {mutant} {family}: err/bound {ratio:.1f}")
    assert ratio > 1.0, (mutant, ratio)


@pytest.mark.parametrize("mutant", ["bsum_off_by_one", "scale_low_bits"])
def test_former_two_percent_rule_accepts_mutant(mutant):
    """The finding behind the oracle, at the shape of test_q40_gemv's middle
    case: the rule `max|want| * 0.02 + 1e-3` against R.q40_matmul passes a
    blocksum that is off by one and weight scales without their two lowest
    mantissa bits; the derived bound rejects both."""
    B, d, n = 4, 128, 1024
    qs, sc, xq, xs, xbs, x = _inputs("natural", d, n, B)
    got = kernel_model(qs, sc, xq, xs, xbs, mutant)
    want = R.q40_matmul(x, R.q40_planes_dequant(qs, sc))
    old_tol = want.abs().max().item() * 0.02 + 1e-3
    old_err = (got - want).abs().max().item()
    ratio = _worst_ratio(got, qs, sc, xq, xs)
    print(f"mutant {mutant}: old err {old_err:.3e} <= old tol {old_tol:.3e}; "
          f"err/bound {ratio:.1f}")
    assert old_err <= old_tol
    assert ratio > 1.0
    clean = kernel_model(qs, sc, xq, xs, xbs)
    assert _worst_ratio(clean, qs, sc, xq, xs) <= 1.0


def _triple(seed=5, rows=3, n=256):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, n, generator=g)
    x[0, 32:64] = 0.0  # an all-zero block: d = 0, codes 0
    return x, R.q80_quantize(x)


def test_q80_emit_check_accepts_reference_quantiser():
    x, (q, s, bs) = _triple()
    R.q80_emit_check(q, s, bs, x.double(), 0.0)
    R.q80_emit_check(q, s, bs, x.double(), torch.zeros_like(x, dtype=torch.float64))


@pytest.mark.parametrize("defect", ["code", "bsum", "scale"])
def test_q80_emit_check_rejects(defect):
    x, (q, s, bs) = _triple()
    q, s, bs = q.clone(), s.clone(), bs.clone()
    if defect == "code":  # one code off by 2, blocksum kept consistent
        i = int((q[1].int().abs() < 100).nonzero()[0])
        q[1, i] += 2
        bs[1, i // 32] += 2
    elif defect == "bsum":
        bs[2, 3] += 1
    else:
        s[1, 2] *= 1.001
    with pytest.raises(AssertionError, match=defect if defect != "bsum" else "blocksum"):
        R.q80_emit_check(q, s, bs, x.double(), 0.0)
