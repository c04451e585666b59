"""Every Q40xQ80 matmul kernel against the exact integer oracle
(reference.q40_q80_exact), every output element within the derived bound
reference.q40_q80_bound, and every Q80 triple producer through
reference.q80_emit_check.

The only tolerances here are that bound, q80_emit_check, and the small
relative terms whose derivation stands beside them. Two input families run
through every kernel: `natural` (quantised Gaussians) and `adversarial`
(dllama_amd.utils.testing.adversarial_q40_q80: saturated nibbles and codes,
negative weight scales, all-zero blocks). Every output buffer is prefilled
with 7.0 and carries one extra row (or slot) that must stay 7.0."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd.ops import reference as R
from dllama_amd.utils.testing import adversarial_q40_q80, natural_q40_planes

DEV = "cuda"
EPS = 1e-5
U = 2.0 ** -24  # f32 unit roundoff
FAMILIES = ("natural", "adversarial")
FILL = 7.0

# worst err / tolerance seen per kernel family; printed at module teardown.
# Informational (how much room the bound leaves), never a threshold.
RATIOS = {}


@pytest.fixture(scope="module")
def k():
    from dllama_amd.ops import hip_ops
    yield hip_ops()
    for name in sorted(RATIOS):
        print(f"\n[err/bound] {name}: {RATIOS[name]:.4f}", end="")
    print()


def rand(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g) * scale


def _q80_bufs(rows, n, guard=0):
    """Q80 triple for `rows` rows plus `guard` extra ones, prefilled with 7."""
    return (torch.full((rows + guard, n), 7, dtype=torch.int8, device=DEV),
            torch.full((rows + guard, n // 32), FILL, device=DEV),
            torch.full((rows + guard, n // 32), FILL, device=DEV))


def _assert_guard(*tails):
    for t in tails:
        assert (t == 7).all(), "write past the end of an output buffer"


@functools.lru_cache(maxsize=None)
def _weights(family, d, n, seed):
    """(qs, sc) on the device."""
    if family == "adversarial":
        qs, sc = adversarial_q40_q80(d, n, 1, 100 + seed)[:2]
    else:
        qs, sc = natural_q40_planes(d, n, 200 + seed)
    return qs.to(DEV), sc.to(DEV)


@functools.lru_cache(maxsize=None)
def _acts(k, family, n, rows, seed):
    """Q80 input triple (xq, xs, xbs) on the device, `rows` rows."""
    if family == "adversarial":
        return tuple(t.to(DEV) for t in adversarial_q40_q80(1, n, rows, 300 + seed)[2:])
    # drawn on the CPU: the same inputs on every machine
    g = torch.Generator().manual_seed(400 + seed)
    x = (torch.randn(rows, n, generator=g) * 0.5).to(DEV)
    out = (torch.zeros(rows, n, dtype=torch.int8, device=DEV),
           torch.zeros(rows, n // 32, device=DEV),
           torch.zeros(rows, n // 32, device=DEV))
    k.q80_quantize(x, *out)
    return out


@functools.lru_cache(maxsize=None)
def _case(k, family, d, n, rows=32, seed=0):
    """(qs, sc, xq, xs, xbs) on the device and the oracle's (y, A) [rows, d].
    Built once per key; nothing may write to any of it."""
    qs, sc = _weights(family, d, n, seed)
    xq, xs, xbs = _acts(k, family, n, rows, seed)
    y, A = R.q40_q80_exact(qs, sc, xq, xs)
    return (qs, sc, xq, xs, xbs), y, A


def _check(name, got, want, tol, what=""):
    """every element: |got - want| <= tol; records the worst err/tol."""
    got = got.detach().cpu().double()
    err = (got - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    worst = ratio.max().item() if ratio.numel() else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), worst)
    assert torch.isfinite(got).all(), (name, what)
    assert (err <= tol).all(), (name, what, worst)


def _ssq_spread(rows, seed):
    """[rows, 16*32] ssq buffer with the row's sum spread over slots 0, 3, 7,
    12 and 15, and its float64 total per row."""
    ssq = torch.zeros(rows, 16 * 32, device=DEV)
    g = torch.Generator().manual_seed(seed)
    for slot in (0, 3, 7, 12, 15):
        ssq[:, slot * 32] = (torch.rand(rows, generator=g) * 9.0 + 1.0).to(DEV)
    total = ssq.cpu().double().reshape(rows, 16, 32)[:, :, 0].sum(-1)
    return ssq, total


def _ssq_total(ssq):
    return ssq.cpu().double().reshape(-1, 16, 32)[:, :, 0].sum(-1)


# 2^-21 * |truth|: the deferred-scale epilogue computes
# rsqrtf(total / n + eps) and multiplies: one rounding each for the divide,
# the add (halved by the root) and the product, the documented 1-2 ulp of
# rsqrtf, and the 4-level f32 tree over the 16 ssq slots (4u, halved): <= 6u.
def _deferred(y, A, nb, total, n):
    inv = torch.rsqrt(total / n + EPS).unsqueeze(-1)
    truth = y * inv
    return truth, R.q40_q80_bound(nb, A) * inv + 2.0 ** -21 * truth.abs()


# ------------------------------------------------------------------ q40_gemv

GEMV_SHAPES = [((69, 32), (1, 2, 4, 8, 16, 32)),
               ((72, 160), (1, 2, 4, 8, 16, 32)),
               # 131 blocks: second trip of the lane stride + trailing block
               ((64, 4192), (1, 2, 4, 8, 16, 32)),
               # RPW 2 at B = 1: half-valid last wave / partial last workgroup
               ((2049, 64), (1,)),
               ((2050, 160), (1,))]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dn,batches", GEMV_SHAPES)
def test_q40_gemv(k, family, dn, batches):
    d, n = dn
    ins, y, A = _case(k, family, d, n)
    for B in batches:
        out = torch.full((B + 1, d), FILL, device=DEV)
        k.q40_gemv(*ins, out, B)
        _check("q40_gemv", out[:B], y[:B], R.q40_q80_bound(n // 32, A[:B]), (d, n, B))
        _assert_guard(out[B])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d,n", [(69, 160), (2050, 64)])
def test_q40_gemv_ssq_in(k, family, d, n):
    ins, y, A = _case(k, family, d, n)
    for B in (1, 2, 4):
        ssq, total = _ssq_spread(B, 10 + B)
        truth, tol = _deferred(y[:B], A[:B], n // 32, total, n)
        out = torch.full((B + 1, d), FILL, device=DEV)
        k.q40_gemv(*ins, out, B, None, ssq, EPS)
        _check("q40_gemv ssq_in", out[:B], truth, tol, (d, n, B))
        _assert_guard(out[B])


def _ksplit_blocks(nb, ks, s):
    """block range of K-slice s: its share of the block PAIRS, and the odd
    trailing block goes to the last slice."""
    nbp = nb // 2
    j0, j1 = 2 * (nbp * s // ks), 2 * (nbp * (s + 1) // ks)
    return j0, (nb if s == ks - 1 else j1)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d,n", [(256, 160), (64, 4192)])
def test_q40_gemv_ksplit(k, family, d, n):
    ins, _, _ = _case(k, family, d, n)
    qs, sc, xq, xs, _ = ins
    nb = n // 32
    for ks in (2, 3, 5):
        part = torch.full((ks + 1, d), FILL, device=DEV)
        k.q40_gemv_ksplit(*ins, part, ks)
        empty = 0
        for s in range(ks):
            j0, j1 = _ksplit_blocks(nb, ks, s)
            ys, As = R.q40_q80_exact(qs, sc, xq[:1], xs[:1], blocks=(j0, j1))
            if j0 == j1:
                empty += 1
                assert (part[s] == 0).all(), (d, n, ks, s)
            _check("q40_gemv_ksplit", part[s:s + 1], ys,
                   R.q40_q80_bound(j1 - j0, As), (d, n, ks, s))
        if n == 160:  # two block pairs: ks = 3 and 5 leave slices empty
            assert empty == {2: 0, 3: 1, 5: 3}[ks]
        _assert_guard(part[ks])


def test_ksplit_blocks_cover():
    for nb, ks in ((5, 2), (5, 3), (5, 5), (131, 2), (131, 3), (131, 5)):
        r = [_ksplit_blocks(nb, ks, s) for s in range(ks)]
        assert r[0][0] == 0 and r[-1][1] == nb
        assert all(a[1] == b[0] for a, b in zip(r, r[1:]))
    # n = 160 with 5 slices: slices 0, 1 and 3 are empty
    assert [_ksplit_blocks(5, 5, s) for s in range(5)] == \
        [(0, 0), (0, 0), (0, 2), (2, 2), (2, 5)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B", [1, 4, 32])
def test_q40_gemv_resid(k, family, B):
    d, n = 69, 160
    ins, y, A = _case(k, family, d, n)
    x0 = rand(B + 1, d, seed=20 + B)
    x0[B] = FILL
    x = x0.clone()
    ssq = torch.zeros(B + 1, 16 * 32, device=DEV)
    k.q40_gemv_resid(*ins, x, ssq, B)
    want = x0[:B].cpu().double() + y[:B]
    # one more f32 add, x0 + y_kernel: u * |x0 + y|
    _check("q40_gemv_resid", x[:B], want,
           R.q40_q80_bound(n // 32, A[:B]) + U * want.abs(), B)
    assert torch.allclose(_ssq_total(ssq)[:B], (want ** 2).sum(-1), rtol=1e-4)
    _assert_guard(x[B])
    assert (ssq[B] == 0).all()


def _resid_q_tol(nb, A, want_x, wnorm):
    """(x tolerance, v_tol of v = x * wnorm): the bound plus the residual
    add's rounding, carried through the product with wnorm (one rounding)."""
    x_tol = R.q40_q80_bound(nb, A) + U * want_x.abs()
    v = want_x * wnorm
    return x_tol, x_tol * wnorm.abs() + U * v.abs(), v


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d,n", [(96, 160), (256, 4192)])
def test_q40_gemv_resid_q(k, family, d, n):
    ins, y, A = _case(k, family, d, n)
    x0 = rand(2, d, seed=30)
    x0[1] = FILL
    wnorm = rand(d, seed=31).abs() + 0.5
    want = x0[:1].cpu().double() + y[:1]
    x_tol, v_tol, v = _resid_q_tol(n // 32, A[:1], want, wnorm.cpu().double())
    try:
        for waves in (4, 8, 16):
            k.q40_gemv_resid_q_waves(waves)
            x, ssq, out = x0.clone(), torch.zeros(2, 16 * 32, device=DEV), _q80_bufs(1, d, 1)
            k.q40_gemv_resid_q(*ins, x, ssq, wnorm, *out)
            _check("q40_gemv_resid_q", x[:1], want, x_tol, (d, n, waves))
            R.q80_emit_check(out[0][:1], out[1][:1], out[2][:1], v, v_tol)
            assert torch.allclose(_ssq_total(ssq)[:1], (want ** 2).sum(-1), rtol=1e-4)
            _assert_guard(x[1], out[0][1], out[1][1], out[2][1])
            assert (ssq[1] == 0).all()
    finally:
        k.q40_gemv_resid_q_waves(0)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d,n", [(96, 160), (256, 4192)])
def test_q40_gemv_pack(k, family, d, n):
    ins, y, A = _case(k, family, d, n)
    nbo = d // 32
    wire = torch.full((2, d + 2 * nbo), 7, dtype=torch.uint8, device=DEV)
    k.q40_gemv_pack(*ins, wire)
    row = wire[0].cpu()
    codes = row[:d].view(torch.int8).reshape(1, d)
    scales = row[d:].contiguous().view(torch.float16).reshape(1, nbo)
    # the wire carries f16(d) and no blocksum
    R.q80_emit_check(codes, scales, None, y[:1], R.q40_q80_bound(n // 32, A[:1]),
                     scale_rtol=2.0 ** -11)
    _assert_guard(wire[1])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", [160, 4192])
def test_add_ssq_q(k, family, n):
    d = 256  # add_ssq_q needs d % 256 == 0
    ins, y, A = _case(k, family, d, n)
    qs, sc, xq, xs, _ = ins
    nb = n // 32
    x0 = rand(2, d, seed=40)
    x0[1] = FILL
    wnorm = rand(d, seed=41).abs() + 0.5
    want = x0[:1].cpu().double() + y[:1]
    for ks in (2, 3):
        part = torch.zeros(ks, d, device=DEV)
        k.q40_gemv_ksplit(*ins, part, ks)
        x, ssq, out = x0.clone(), torch.zeros(2, 16 * 32, device=DEV), _q80_bufs(1, d, 1)
        k.add_ssq_q(x[0], part, ssq, wnorm, *(t[0] for t in out), ks)
        # each slice within its own bound, then the chain x0 + part[0] + ..:
        # ks f32 adds, each rounding a partial sum of at most |x0| + A
        x_tol = sum(R.q40_q80_bound(j1 - j0, R.q40_q80_exact(
            qs, sc, xq[:1], xs[:1], blocks=(j0, j1))[1])
            for j0, j1 in (_ksplit_blocks(nb, ks, s) for s in range(ks)))
        x_tol = x_tol + ks * U * (x0[:1].cpu().double().abs() + A[:1])
        _check("add_ssq_q", x[:1], want, x_tol, (n, ks))
        wn = wnorm.cpu().double()
        v = want * wn
        R.q80_emit_check(out[0][:1], out[1][:1], out[2][:1], v,
                         x_tol * wn.abs() + U * v.abs())
        assert torch.allclose(_ssq_total(ssq)[:1], (want ** 2).sum(-1), rtol=1e-4)
        _assert_guard(x[1], out[0][1], out[1][1], out[2][1])


# -------------------------------------------------------------------- argmax

def _argmax_run(k, qs, sc, xq, xs, xbs):
    d = qs.shape[0]
    nblocks = int(k.q40_gemv_argmax_blocks(d))
    scratch = torch.zeros(nblocks + 1, dtype=torch.int64, device=DEV)
    scratch[nblocks] = 7
    out = torch.full((2, d), FILL, device=DEV)
    k.q40_gemv(qs, sc, xq, xs, xbs, out, 1, scratch)
    tok = torch.full((2,), 7, dtype=torch.int64, device=DEV)
    k.token_from_argmax(tok, scratch, nblocks)
    _assert_guard(out[1], scratch[nblocks], tok[1])
    return int(tok[0].item()), out[:1]


def _argmax_expect(qs, sc, xq, xs):
    """(first maximum of the oracle's y, valid): valid when the maximum
    leads every smaller value by more than the two bounds together. Rows
    with an identical oracle value are identical weight rows here (planted),
    which every kernel computes to the same f32."""
    y, A = R.q40_q80_exact(qs, sc, xq, xs)
    y, A = y[0], A[0]
    bound = R.q40_q80_bound(xs.shape[-1], A)
    m = y.max()
    first = int((y == m).nonzero()[0])
    rest = y < m
    gap_ok = bool(((m - y[rest]) > (bound[first] + bound[rest])).all())
    return first, gap_ok, y, A


ARGMAX_D = [512, 2050]  # RPW 1 / RPW 2 (4 / 8 rows per workgroup)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d", ARGMAX_D)
def test_gemv_argmax(k, family, d):
    n = 256
    (qs, sc, xq, xs, xbs), _, _ = _case(k, family, d, n, rows=1, seed=7)
    first, valid, y, A = _argmax_expect(qs, sc, xq, xs)
    assert valid, "pick another seed: the top two are within twice the bound"
    tok, out = _argmax_run(k, qs, sc, xq, xs, xbs)
    _check("q40_gemv argmax y", out, y[None], R.q40_q80_bound(n // 32, A[None]), d)
    assert tok == first


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d", ARGMAX_D)
def test_gemv_argmax_all_negative(k, family, d):
    """Every logit below zero: argmax_pack orders negatives by flipping all
    bits, positives by setting the sign bit."""
    n = 256
    (qs, sc, xq, xs, xbs), y, _ = _case(k, family, d, n, rows=1, seed=7)
    sc = torch.where((y[0] > 0).to(DEV).unsqueeze(-1), -sc, sc)  # negates y[row] exactly
    first, valid, y2, _ = _argmax_expect(qs, sc, xq, xs)
    assert (y2 <= 0).all() and (y2 < 0).sum() >= d - 2
    assert valid, "pick another seed: the top two are within twice the bound"
    tok, _ = _argmax_run(k, qs, sc, xq, xs, xbs)
    assert tok == first


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d", ARGMAX_D)
@pytest.mark.parametrize("where", ["waves", "workgroups"])
def test_gemv_argmax_ties(k, family, d, where):
    """The maximal weight row planted at two indices: the smaller one wins,
    across the waves of one workgroup and across workgroups."""
    n = 256
    (qs, sc, xq, xs, xbs), y, _ = _case(k, family, d, n, rows=1, seed=7)
    rows_per_wg = 4 if d < 2048 else 8
    if where == "waves":  # one workgroup, different waves
        i1, i2 = 5 * rows_per_wg + 1, 5 * rows_per_wg + rows_per_wg // 2 + 1
    else:
        i1, i2 = 3 * rows_per_wg + 2, 40 * rows_per_wg + rows_per_wg - 3
    top, low = int(y[0].argmax()), int(y[0].argmin())
    qs, sc = qs.clone(), sc.clone()
    for i in (i1, i2):
        qs[i], sc[i] = qs[top], sc[top]
    if top not in (i1, i2):  # the original goes, so exactly two rows tie
        qs[top], sc[top] = qs[low], sc[low]
    first, valid, y2, _ = _argmax_expect(qs, sc, xq, xs)
    assert first == i1 and y2[i2] == y2[i1] and (y2 == y2.max()).sum() == 2
    assert valid, "pick another seed: the runner-up is within twice the bound"
    tok, out = _argmax_run(k, qs, sc, xq, xs, xbs)
    assert out[0, i1] == out[0, i2]
    assert tok == i1


# ------------------------------------------------------------------ q40_gemm

@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d,n,batch", [(8, 32, 1), (129, 160, 20),
                                       # 9 blocks: v2's second chunk of one
                                       # block, v1's odd tail
                                       (160, 288, 32), (256, 4192, 9)])
def test_q40_gemm(k, family, d, n, batch):
    """Rows batch..31 of xq / xs hold live data of other rows (non-zero in
    both families) and must not reach y."""
    (qs, sc, xq, xs, _), y, A = _case(k, family, d, n)
    assert xq[batch:].ne(0).any() or batch == 32
    tol = R.q40_q80_bound(n // 32, A[:batch])
    for variant in (0, 1):
        for use_part in (False, True):
            part = torch.full((16 * 32 * d + 1,), FILL, device=DEV) if use_part else None
            out = torch.full((batch + 1, d), FILL, device=DEV)
            k.q40_gemm(qs, sc, xq, xs, out, batch,
                       part[:16 * 32 * d] if use_part else None, variant=variant)
            _check(f"q40_gemm v{variant + 1}", out[:batch], y[:batch], tol,
                   (d, n, batch, variant, use_part))
            _assert_guard(out[batch])
            if use_part:
                _assert_guard(part[16 * 32 * d])


# ---------------------------------------------------------- q40_gemv_grouped

E, GB, KA = 4, 2, 2
IDX = [3, 0, 3, 1]  # a repeated expert, not monotonic
# top-2 of row 0 is (1, 3), of row 1 (0, 3); every gap in the sorted logits
# is at least 0.1
ROUTER = [[0.3, 1.5, -0.7, 0.9], [2.0, -1.0, 0.5, 1.2]]


@functools.lru_cache(maxsize=None)
def _grouped_case(k, family, d, n):
    """stacked expert planes [E, d, ..], the shared input triple, and the
    oracle per expert: y, A [E, GB, d]."""
    ws = [_weights(family, d, n, 50 + e) for e in range(E)]
    qs = torch.stack([w[0] for w in ws])
    sc = torch.stack([w[1] for w in ws])
    xq, xs, xbs = _acts(k, family, n, GB, 60)
    ya = [R.q40_q80_exact(w[0], w[1], xq, xs) for w in ws]
    return (qs, sc, xq, xs, xbs), torch.stack([t[0] for t in ya]), \
        torch.stack([t[1] for t in ya])


def _slots(y, A, experts):
    """oracle rows of the slots: slot s = (row s // KA, expert experts[s])."""
    sel = [(e, s // KA) for s, e in enumerate(experts)]
    return (torch.stack([y[e, b] for e, b in sel]),
            torch.stack([A[e, b] for e, b in sel]))


def test_router_fixture():
    logits = torch.tensor(ROUTER)
    srt = logits.sort(dim=-1, descending=True).values
    assert ((srt[:, :-1] - srt[:, 1:]) >= 0.1 - 1e-6).all()
    idx, _ = R.moe_gate(logits, KA)
    assert idx.tolist() == [[1, 3], [0, 3]]


@pytest.mark.parametrize("family", FAMILIES)
# LPP 8, 8, 16, 64, 64 with a second trip
@pytest.mark.parametrize("n", [32, 160, 768, 2112, 4192])
def test_q40_gemv_grouped(k, family, n):
    nb = n // 32
    S = GB * KA
    for d in (69, 96):
        ins, y, A = _grouped_case(k, family, d, n)
        idx = torch.tensor(IDX, dtype=torch.int32, device=DEV)
        ys, As = _slots(y, A, IDX)
        router = torch.tensor(ROUTER, device=DEV)
        gated = R.moe_gate(router.cpu(), KA)[0].reshape(-1).tolist()
        yg, Ag = _slots(y, A, gated)
        ssq, total = _ssq_spread(GB, 70)
        slot_total = total.repeat_interleave(KA)
        for variant in (0, 1):
            name = f"q40_gemv_grouped v{variant + 1}"
            out = torch.full((S + 1, d), FILL, device=DEV)
            k.q40_gemv_grouped(*ins, idx, out, KA, variant=variant)
            _check(name, out[:S], ys, R.q40_q80_bound(nb, As), (d, n))
            _assert_guard(out[S])
            out = torch.full((S + 1, d), FILL, device=DEV)
            k.q40_gemv_grouped(*ins, idx, out, KA, variant=variant, ssq_in=ssq, eps=EPS)
            truth, tol = _deferred(ys, As, nb, slot_total, n)
            _check(name + " ssq_in", out[:S], truth, tol, (d, n))
            _assert_guard(out[S])
            out = torch.full((S + 1, d), FILL, device=DEV)
            k.q40_gemv_grouped(*ins, torch.zeros_like(idx), out, KA, variant=variant,
                               router=router, topk=KA, n_slots=S)
            _check(name + " router", out[:S], yg, R.q40_q80_bound(nb, Ag), (d, n))
            _assert_guard(out[S])


@pytest.mark.parametrize("family", FAMILIES)
def test_q40_gemv_grouped_partial_wave(k, family):
    """d = 66 with 8 lanes per row pair: in the last wave only lanes 0..7 own
    a row. The in-kernel gate and the ssq total shuffle across the whole
    wave, so those lanes still need what the other 56 hold: 128 experts sit
    two per lane with the winners in lanes 16..60, and the ssq slots 12 and
    15 are read by lanes 12 and 15."""
    d, n, ne = 66, 160, 128
    nb, S = n // 32, GB * KA
    if family == "adversarial":
        qs, sc = adversarial_q40_q80(ne * d, n, 1, 90)[:2]
    else:
        qs, sc = natural_q40_planes(ne * d, n, 91)
    qs, sc = qs.reshape(ne, d, n // 2).to(DEV), sc.reshape(ne, d, nb).to(DEV)
    xq, xs, xbs = _acts(k, family, n, GB, 92)
    want = [[77, 120], [33, 101]]
    logits = torch.linspace(-3.0, -1.0, ne).repeat(GB, 1)
    for b, (e0, e1) in enumerate(want):
        logits[b, e0], logits[b, e1] = 2.0, 1.0
    assert R.moe_gate(logits, KA)[0].tolist() == want
    experts = [e for row in want for e in row]
    ya = [R.q40_q80_exact(qs[e], sc[e], xq[s // KA:s // KA + 1], xs[s // KA:s // KA + 1])
          for s, e in enumerate(experts)]
    ys, As = torch.cat([t[0] for t in ya]), torch.cat([t[1] for t in ya])
    idx = torch.tensor(experts, dtype=torch.int32, device=DEV)
    router = logits.to(DEV)
    ssq, total = _ssq_spread(GB, 93)
    truth, tol = _deferred(ys, As, nb, total.repeat_interleave(KA), n)
    for variant in (0, 1):
        name = f"q40_gemv_grouped v{variant + 1}"
        out = torch.full((S + 1, d), FILL, device=DEV)
        k.q40_gemv_grouped(qs, sc, xq, xs, xbs, idx, out, KA, variant=variant,
                           ssq_in=ssq, eps=EPS)
        _check(name + " ssq_in", out[:S], truth, tol, (d, n))
        _assert_guard(out[S])
        out = torch.full((S + 1, d), FILL, device=DEV)
        k.q40_gemv_grouped(qs, sc, xq, xs, xbs, torch.zeros_like(idx), out, KA,
                           variant=variant, router=router, topk=KA, n_slots=S)
        _check(name + " router", out[:S], ys, R.q40_q80_bound(nb, As), (d, n))
        _assert_guard(out[S])


# ------------------------------------------------------- SwiGLU-fused GEMVs

def _act64(a, gelu):
    if gelu:
        return 0.5 * a * (1.0 + torch.tanh(0.797884560802865 * (a + 0.044715 * a ** 3)))
    return a * torch.sigmoid(a)


def _swiglu_truth(ya, Aa, yg, Ag, nb, gelu):
    """v = act(a) * g and its v_tol: the error of a (at most bound_a) passes
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
@pytest.mark.parametrize("n", [160, 4192])
def test_q40_gemv_swiglu(k, family, gelu, n):
    for ff in (32, 96):
        ins, y, A = _case(k, family, 2 * ff, n, rows=1, seed=3)
        v, v_tol = _swiglu_truth(y[:, :ff], A[:, :ff], y[:, ff:], A[:, ff:], n // 32, gelu)
        out = tuple(t.reshape(-1) for t in _q80_bufs(1, ff, 1))
        k.q40_gemv_swiglu(*ins, *out, gelu)
        nbo = ff // 32
        R.q80_emit_check(out[0][:ff].reshape(1, ff), out[1][:nbo].reshape(1, nbo),
                         out[2][:nbo].reshape(1, nbo), v, v_tol)
        _assert_guard(out[0][ff:], out[1][nbo:], out[2][nbo:])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("n", [160, 4192])
def test_q40_gemv_grouped_swiglu(k, family, gelu, n):
    S = GB * KA
    router = torch.tensor(ROUTER, device=DEV)
    gated = R.moe_gate(router.cpu(), KA)[0].reshape(-1).tolist()
    for ff in (32, 96):
        ins, y, A = _grouped_case(k, family, 2 * ff, n)
        ys, As = _slots(y, A, gated)
        v, v_tol = _swiglu_truth(ys[:, :ff], As[:, :ff], ys[:, ff:], As[:, ff:],
                                 n // 32, gelu)
        out = _q80_bufs(S, ff, 1)
        k.q40_gemv_grouped_swiglu(*ins, *out, S, router, KA, gelu)
        R.q80_emit_check(out[0][:S], out[1][:S], out[2][:S], v, v_tol)
        _assert_guard(out[0][S], out[1][S], out[2][S])


# ------------------------------------------- every other Q80 triple producer
# q80_emit_check against the float64 value of what the op quantises, at the
# smallest shape of the op's test in test_hip_ops.py. The older, looser
# checks stay where they are; these add the exact blocksum and the d/2 code
# check.

# rmsnorm kernels that reduce x^2 themselves: v = x * inv * w with
# inv = rsqrtf(ssq / n + eps). ssq is a sum of non-negative f32 terms, each
# squared (1 rounding) and passing through at most DEPTH additions (serial
# per-thread strides, 6 wave levels, up to 16 serial wave partials: 4 + 6 +
# 16 at most in either kernel), so its relative error is at most
# (DEPTH + 1) u; the divide and the add of eps round once each; the root
# halves all of that; rsqrtf is good to 2 ulp; two products follow.
_NORM_DEPTH = 26
_NORM_RTOL = (0.5 * (_NORM_DEPTH + 3) + 2 + 2) * U


def _rms64(x, w, eps):
    x = x.cpu().double()
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w.cpu().double()


def test_q80_quantize_emit(k):
    x = rand(5, 4096, seed=1)
    x[4] = FILL
    x[1, 64:96] = 0.0  # an all-zero block: scale 0, codes 0
    out = _q80_bufs(4, 4096, 1)
    k.q80_quantize(x[:4], *(t[:4] for t in out))
    R.q80_emit_check(out[0][:4], out[1][:4], out[2][:4], x[:4].cpu().double(), 0.0)
    assert (out[1][1, 2] == 0) and (out[0][1, 64:96] == 0).all()
    _assert_guard(out[0][4], out[1][4], out[2][4])


def test_rmsnorm_q80_emit(k):
    x = rand(2, 1024, seed=4)
    w = rand(1024, seed=5).abs()
    out = _q80_bufs(2, 1024, 1)
    k.rmsnorm_q80(x, w, *(t[:2] for t in out), EPS)
    v = _rms64(x, w, EPS)
    R.q80_emit_check(out[0][:2], out[1][:2], out[2][:2], v, _NORM_RTOL * v.abs())
    _assert_guard(out[0][2], out[1][2], out[2][2])


def test_add_rmsnorm_q80_emit(k):
    x = rand(2, 4096, seed=83)
    p = rand(2, 4096, seed=84)
    w = rand(4096, seed=85).abs()
    out = _q80_bufs(2, 4096, 1)
    xs = x.clone()
    k.add_rmsnorm_q80(xs, p, w, *(t[:2] for t in out), EPS)
    assert torch.equal(xs, x + p)  # one correctly rounded f32 add
    v = _rms64(xs, w, EPS)
    R.q80_emit_check(out[0][:2], out[1][:2], out[2][:2], v, _NORM_RTOL * v.abs())
    _assert_guard(out[0][2], out[1][2], out[2][2])


@pytest.mark.parametrize("gelu,n", [(False, 512), (True, 256)])
def test_swiglu_q80_emit(k, gelu, n):
    a = rand(2, n, seed=190 if gelu else 80)
    g = rand(2, n, seed=191 if gelu else 81)
    out = _q80_bufs(2, n, 1)
    k.swiglu_q80(a, g, n, n, 2, *(t[:2] for t in out), gelu)
    a64, g64 = a.cpu().double(), g.cpu().double()
    v = _act64(a64, gelu) * g64
    if gelu:
        # 0.5*a*(1 + tanhf(z)): tanhf is good to 2 ulp of a value below 1
        # (2^-23 absolute), z's own error (4 roundings) passes through
        # tanh' <= 1 scaled by |z|(1 - tanh^2) <= 0.45, together at most
        # 2^-22 absolute on (1 + tanh); then the sum, two products inside
        # and the product with g round once each: 4u relative
        v_tol = 2.0 ** -22 * (0.5 * a64 * g64).abs() + 4 * U * v.abs()
    else:
        # a / (1 + __expf(-a)) * g: __expf is exp2(-a * log2e), whose
        # argument rounding gives |a| u relative and the instruction 1 ulp
        # (both scaled by e/(1+e) <= 1); the add rounds once, the divide is
        # good to 2.5 ulp, the product with g rounds once
        v_tol = (a64.abs() + 6) * U * v.abs()
    R.q80_emit_check(out[0][:2], out[1][:2], out[2][:2], v, v_tol)
    _assert_guard(out[0][2], out[1][2], out[2][2])


@pytest.mark.parametrize("deferred", [False, True])
def test_norm_quant_emit(k, deferred):
    B, n = 1, 160
    x = rand(B, n, seed=620 + n)
    w = rand(n, seed=621).abs() + 0.5
    ssq, total = _ssq_spread(B, 80)
    out = _q80_bufs(B, n, 1)
    yout = torch.full((B + 1, n), FILL, device=DEV)
    k.norm_quant(x, w, ssq, *(t[:B] for t in out), B, EPS, yout, deferred)
    x64, w64 = x.cpu().double(), w.cpu().double()
    if deferred:  # x * 1.0f * w: one rounding
        v, rtol = x64 * w64, U
    else:
        # rsqrtf(total / n + eps): 15 serial f32 adds of the non-negative
        # slots, the divide and the add (all halved by the root), 2 ulp of
        # rsqrtf, then two products
        v = x64 * torch.rsqrt(total / n + EPS).unsqueeze(-1) * w64
        rtol = (0.5 * 17 + 2 + 2) * U
    R.q80_emit_check(out[0][:B], out[1][:B], out[2][:B], v, rtol * v.abs())
    _check("norm_quant yout", yout[:B], v, rtol * v.abs(), deferred)
    _assert_guard(out[0][B], out[1][B], out[2][B], yout[B])


def _wire_bytes(n):
    return n + 2 * (n // 32)


def test_merge_add_q_emit(k):
    rows, n, world = 1, 256, 2
    bufs = torch.zeros(world, rows, _wire_bytes(n), dtype=torch.uint8, device=DEV)
    for w in range(world):
        k.sync_quant_pack(rand(rows, n, seed=650 + w), bufs[w])
    x = rand(rows + 1, n, seed=653)
    x[rows] = FILL
    wnorm = rand(n, seed=654).abs() + 0.5
    ssq, out = torch.zeros(rows + 1, 16 * 32, device=DEV), _q80_bufs(rows, n, 1)
    k.merge_add_q(x[:rows], bufs, ssq, wnorm, *(t[:rows] for t in out))
    # the op quantises x_out * wnorm, x_out being the f32 it stored
    v = x[:rows].cpu().double() * wnorm.cpu().double()
    R.q80_emit_check(out[0][:rows], out[1][:rows], out[2][:rows], v, U * v.abs())
    _assert_guard(x[rows], out[0][rows], out[1][rows], out[2][rows])


def test_scale_merge_add_q_emit(k):
    rows, n, topk = 1, 256, 2
    y = rand(rows * topk, n, seed=670)
    wts = rand(rows, topk, seed=671).abs()
    x = rand(rows + 1, n, seed=672)
    x[rows] = FILL
    wnorm = rand(n, seed=673).abs() + 0.5
    ssq, out = torch.zeros(rows + 1, 16 * 32, device=DEV), _q80_bufs(rows, n, 1)
    k.scale_merge_add_q(x[:rows], y, wts, ssq, wnorm, *(t[:rows] for t in out), rows, topk)
    v = x[:rows].cpu().double() * wnorm.cpu().double()
    R.q80_emit_check(out[0][:rows], out[1][:rows], out[2][:rows], v, U * v.abs())
    _assert_guard(x[rows], out[0][rows], out[1][rows], out[2][rows])
