"""logprob_rows (csrc/logprob.hip) against the float64 oracle
logprob_rows_ref on the same f32 logits.

Ids must be equal exactly: kernel and oracle see identical inputs and the
order (descending value, lower index first, -0.0 equal to +0.0) is total.

Log-probabilities must be within 2e-5 absolute for rows whose finite entries
spread over at most 64: `logit - max` rounds to half an ulp of at most 64
(3.8e-6), log(S) carries the relative error of about 24 dependent f32
operations on expf values (about 3e-6 at these sizes), and the bound leaves
about 3x over their sum. The kernel computes (logit - max) - log(S), so the
bound holds wherever the logits sit (the rows shifted by +-1e4).

lse is held to the same 2e-5 plus one f32 spacing at |lse|: it is an f32
output of the size of the logits themselves, and f32 cannot carry 1e4 to
better than 4.9e-4. For unshifted rows (|lse| < 32) that term is below 2e-6.

Largest errors seen on an MI355X are in profiles/r11_logprobs.md.
"""

import numpy as np
import pytest
import torch

from dllama_amd.ops import hip_ops
from dllama_amd.ops.reference import logprob_rows_ref

pytestmark = pytest.mark.gpu

TOL = 2e-5
VOCABS = [7, 33, 1000, 1024, 1025, 4096, 70001, 151936]
NEG_INF = float("-inf")
worst = {"logprob": 0.0, "lse": 0.0}  # printed by the last test


@pytest.fixture(scope="module")
def k():
    return hip_ops()


def _randn(b, v, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, v, generator=g) * 3


def _targets(b, v, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    t = torch.randint(0, v, (b,), generator=g)
    # the edges: first, last, none, one past the end
    for i, edge in enumerate((0, v - 1, -1, v)):
        if i < b:
            t[i] = edge
    return t


def _special_rows(v):
    """One row per hazard, all in one batch."""
    base = _randn(8, v, 7)
    rows = []
    rows.append(base[0] + 1e4)            # the max must be subtracted
    rows.append(base[1] - 1e4)
    rows.append(torch.full((v,), 1.25))   # constant: ids 0..k-1, all -log V
    tie = base[2].clone()                 # equal maxima across a chunk boundary
    lo = min(1023, v - 2)
    tie[lo] = tie[lo + 1] = tie.max() + 1.0
    rows.append(tie)
    zeros = -base[3].abs() - 0.1          # -0.0 and +0.0 the two largest
    zeros[2], zeros[v - 2] = -0.0, 0.0    # equal: the lower index leads
    rows.append(zeros)
    half = base[4].clone()                # half the entries -inf, interleaved
    half[::2] = NEG_INF
    rows.append(half)
    block = base[5].clone()               # ... and in whole chunks
    block[: v // 2] = NEG_INF
    rows.append(block)
    dup = base[6].clone()                 # many equal values inside the top list
    dup[torch.arange(0, v, 3)] = dup.max()
    rows.append(dup)
    return torch.stack(rows)


def _launch(k, logits, v, targets, kk):
    b = logits.shape[0] if logits.dim() == 2 else 1
    n = b * int(k.logprob_chunks(v))
    dev = logits.device
    # poisoned scratch and outputs: nothing stale may show
    part = torch.full((2 * n,), float("nan"), device=dev)
    keys = torch.full((20 * n,), -1, dtype=torch.int64, device=dev)
    out_lp = torch.full((b, 22), float("nan"), device=dev)
    out_id = torch.full((b, 20), -7, dtype=torch.int32, device=dev)
    k.logprob_rows(logits, v, targets, kk, part, keys, out_lp, out_id)
    return out_lp, out_id


def _close(got, want, tol):
    """|got - want| <= tol where finite, equal where infinite; the largest
    finite error."""
    got, want = got.double(), want.double()
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf])
    err = (got[~inf] - want[~inf]).abs()
    assert not torch.isnan(err).any()
    worst_here = float(err.max()) if err.numel() else 0.0
    assert (err <= (tol[~inf] if torch.is_tensor(tol) else tol)).all(), worst_here
    return worst_here


def _check(k, x, v, targets, kk, ref, dev_logits=None, dev_targets=None):
    """x: CPU f32 [B, v]; ref: logprob_rows_ref(x, targets, 20), shared by
    every k (a shorter list is its prefix)."""
    lse, lp, top_lp, top_id = ref
    want_lp, want_id = top_lp.clone(), top_id.clone()
    want_lp[:, kk:] = NEG_INF
    want_id[:, kk:] = -1
    out_lp, out_id = _launch(
        k, x.cuda() if dev_logits is None else dev_logits, v,
        targets.cuda() if dev_targets is None else dev_targets, kk)
    out_lp, out_id = out_lp.cpu(), out_id.cpu()
    assert torch.equal(out_id.long(), want_id)  # exactly, no case left out
    spread = torch.where(torch.isinf(x), torch.nan, x.double())
    spread = np.nanmax(spread.numpy(), 1) - np.nanmin(spread.numpy(), 1)
    assert (spread <= 64).all()
    e1 = _close(out_lp[:, 1], lp, TOL)
    e2 = _close(out_lp[:, 2:], want_lp, TOL)
    spacing = torch.from_numpy(np.spacing(lse.abs().float().numpy())).double()
    e0 = _close(out_lp[:, 0], lse, TOL + spacing)
    worst["logprob"] = max(worst["logprob"], e1, e2)
    worst["lse"] = max(worst["lse"], e0)
    print(f"V={v} B={x.shape[0]} k={kk}: max |err| logprob {max(e1, e2):.3g} "
          f"lse {e0:.3g}")


@pytest.mark.parametrize("v", VOCABS)
def test_random_rows(k, v):
    for b in (1, 3, 32):
        x, t = _randn(b, v, 10 + b), _targets(b, v, b)
        ref = logprob_rows_ref(x, t, 20)
        for kk in (0, 1, 5, 20):  # v = 7 at k = 20: the -1 / -inf padding
            _check(k, x, v, t, kk, ref)


@pytest.mark.parametrize("v", VOCABS)
def test_special_rows(k, v):
    x = _special_rows(v)
    t = _targets(x.shape[0], v, 3)
    t[4], t[5] = 2, 0  # the -0.0 entry; an entry that is -inf
    ref = logprob_rows_ref(x, t, 20)
    for kk in (5, 20):
        _check(k, x, v, t, kk, ref)
    top_lp, top_id = ref[2], ref[3]
    n = min(20, v)
    assert top_id[2, :n].tolist() == list(range(n))       # constant row
    assert np.allclose(top_lp[2, :n], -np.log(v), atol=1e-12)
    lo = min(1023, v - 2)
    assert top_id[3, :2].tolist() == [lo, lo + 1]          # chunk-boundary tie
    assert top_id[4, :2].tolist() == [2, v - 2]            # -0.0 before +0.0


@pytest.mark.parametrize("v", [1000, 4096, 70001])
def test_row_stride_and_strided_targets(k, v):
    """The row stride is larger than V with large positive garbage beyond V,
    which must not be read; the targets are every other element."""
    b = 3
    x, t = _randn(b, v, 21), _targets(b, v, 4)
    wide = torch.full((b, v + 37), 3e38)
    wide[:, :v] = x
    dev = wide.cuda()[:, :v]
    assert dev.stride(0) == v + 37 and not dev.is_contiguous()
    pairs = torch.stack([t, torch.full_like(t, v + 5)], 1).cuda()
    ref = logprob_rows_ref(x, t, 20)
    _check(k, x, v, t, 20, ref, dev_logits=dev, dev_targets=pairs[:, 0])
    # a 1-D row with a one-element target view, as sample_out[0:1] is passed
    _check(k, x[1:2], v, t[1:2], 5, tuple(r[1:2] for r in ref),
           dev_logits=dev[1], dev_targets=pairs[1, 0:1])


def test_same_input_same_bits(k):
    v = 70001
    x, t = _randn(32, v, 5).cuda(), _targets(32, v, 5).cuda()
    a_lp, a_id = _launch(k, x, v, t, 20)
    b_lp, b_id = _launch(k, x, v, t, 20)
    assert torch.equal(a_lp.view(torch.int32), b_lp.view(torch.int32))
    assert torch.equal(a_id, b_id)


def test_captured_launches_follow_new_contents(k):
    v, b = 4096, 3
    x, t = _randn(b, v, 31).cuda(), _targets(b, v, 6).cuda()
    n = b * int(k.logprob_chunks(v))
    part = torch.zeros(2 * n, device="cuda")
    keys = torch.zeros(20 * n, dtype=torch.int64, device="cuda")
    out_lp = torch.zeros(b, 22, device="cuda")
    out_id = torch.zeros(b, 20, dtype=torch.int32, device="cuda")

    def body():
        k.logprob_rows(x, v, t, 20, part, keys, out_lp, out_id)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    x2, t2 = _randn(b, v, 32), _targets(b, v, 7).flip(0)
    x.copy_(x2)
    t.copy_(t2)
    g.replay()
    lse, lp, top_lp, top_id = logprob_rows_ref(x2, t2, 20)
    assert torch.equal(out_id.cpu().long(), top_id)
    _close(out_lp[:, 1].cpu(), lp, TOL)
    _close(out_lp[:, 2:].cpu(), top_lp, TOL)
    _close(out_lp[:, 0].cpu(), lse, TOL)


def test_limits_are_checked(k):
    x, t = _randn(1, 64, 1).cuda(), torch.zeros(1, dtype=torch.int64).cuda()
    with pytest.raises(RuntimeError, match="k must be 0..20"):
        _launch(k, x, 64, t, 21)
    with pytest.raises(RuntimeError, match="vocab_size"):
        _launch(k, x, 1, t, 1)
    with pytest.raises(RuntimeError, match="vocab_size"):
        _launch(k, x, 65, t, 1)  # more than the row holds
    with pytest.raises(RuntimeError, match="unit element stride"):
        _launch(k, _randn(2, 64, 1).cuda()[:, ::2], 32, t.repeat(2), 1)
    # every preset vocabulary and 2^18 fit at k = 20; past the chunk-key
    # limit the call is refused with the limit named, and k = 0 still runs
    assert int(k.logprob_chunks(1 << 18)) * 20 <= 6144
    v = 6144 // 20 * 1024 + 1
    big = torch.zeros(v, device="cuda")
    with pytest.raises(RuntimeError, match="at most 6144 chunk keys"):
        _launch(k, big, v, t, 20)
    out_lp, _ = _launch(k, big, v, t, 0)
    assert abs(float(out_lp[0, 0]) - np.log(v)) < TOL


def test_zz_report_worst_error():
    print(f"largest |error| over this file: logprob {worst['logprob']:.3g}, "
          f"lse {worst['lse']:.3g}")
    assert worst["logprob"] <= TOL
