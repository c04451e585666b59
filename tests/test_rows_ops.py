"""Row-table forms of the positional kernels (rope_kv_rows,
rope_kv_qknorm_rows, attn_rows, rows_advance): with the table {0, p0+b} they
are the single-sequence kernels bit for bit; with a ragged table every row
ropes, writes and attends inside its own KV slot and nowhere else."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd.ops import reference as R

DEV = "cuda"
KV_DTYPES = [torch.float32, torch.float16]


@pytest.fixture(scope="module")
def k():
    from dllama_amd.ops import hip_ops
    return hip_ops()


def rand(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g) * scale


def table(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


def rope_cache(seq, hd):
    return R.rope_cache(seq, hd, 10000.0).to(DEV).reshape(seq, hd).contiguous()


# ------------------------------------------------ equivalence: table {0, p0+b}

@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("style", [0, 1])
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_kv_rows_equals_rope_kv(k, style, kv_dt, hd):
    B, qh, kvh, seq, p0 = 3, 4, 2, 32, 7
    q_dim0, kv_dim0 = qh * hd, kvh * hd
    ld = q_dim0 + 2 * kv_dim0
    buf = rand(B, ld, seed=500 + hd)
    buf_r = buf.clone()
    cache = rope_cache(seq, hd)
    kc, vc, kc_r, vc_r = (torch.zeros(seq, kv_dim0, dtype=kv_dt, device=DEV)
                          for _ in range(4))
    pos = torch.tensor([p0], dtype=torch.int32, device=DEV)
    k.rope_kv(buf, ld, q_dim0, kv_dim0, cache, pos, kc, vc, hd, style, B)
    k.rope_kv_rows(buf_r, ld, q_dim0, kv_dim0, cache,
                   table([[0, p0 + b] for b in range(B)]), kc_r, vc_r, hd,
                   style, B)
    assert torch.equal(buf_r, buf)
    assert torch.equal(kc_r, kc) and torch.equal(vc_r, vc)
    assert kc[p0: p0 + B].abs().sum() > 0


@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_kv_qknorm_rows_equals_rope_kv_qknorm(k, kv_dt, hd):
    B, qh, kvh, seq, p0 = 3, 4, 2, 32, 9
    q_dim0, kv_dim0 = qh * hd, kvh * hd
    ld = q_dim0 + 2 * kv_dim0
    buf = rand(B, ld, seed=510 + hd)
    buf_r = buf.clone()
    wq = rand(hd, seed=511).abs() + 0.5
    wk = rand(hd, seed=512).abs() + 0.5
    cache = rope_cache(seq, hd)
    kc, vc, kc_r, vc_r = (torch.zeros(seq, kv_dim0, dtype=kv_dt, device=DEV)
                          for _ in range(4))
    pos = torch.tensor([p0], dtype=torch.int32, device=DEV)
    k.rope_kv_qknorm(buf, ld, q_dim0, kv_dim0, cache, pos, kc, vc, hd, wq, wk,
                     1e-6, B)
    k.rope_kv_qknorm_rows(buf_r, ld, q_dim0, kv_dim0, cache,
                          table([[0, p0 + b] for b in range(B)]), kc_r, vc_r,
                          hd, wq, wk, 1e-6, B)
    assert torch.equal(buf_r, buf)
    assert torch.equal(kc_r, kc) and torch.equal(vc_r, vc)


def _attn_bufs(B, H0, hd, S):
    return (torch.zeros(B * H0 * S * 2, device=DEV),
            torch.zeros(B * H0 * S * hd, device=DEV))


def _q80_bufs(B, H0, hd):
    nb = H0 * hd // 32
    return (torch.zeros(B, H0 * hd, dtype=torch.int8, device=DEV),
            torch.zeros(B, nb, device=DEV), torch.zeros(B, nb, device=DEV))


@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("S", [8, 16])
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_rows_equals_attn(k, hd, S, kv_dt):
    B, H0, n_kv0, seq, p0 = 3, 4, 2, 300, 250
    kv_dim0 = n_kv0 * hd
    kc = rand(seq, kv_dim0, seed=520 + hd, scale=0.3).to(kv_dt)
    vc = rand(seq, kv_dim0, seed=521 + hd).to(kv_dt)
    q = rand(B, H0 * hd, seed=522)
    pos = torch.tensor([p0], dtype=torch.int32, device=DEV)
    rows = table([[0, p0 + b] for b in range(B)])
    cnt = torch.zeros(B * H0, dtype=torch.int32, device=DEV)
    ml, osc = _attn_bufs(B, H0, hd, S)
    y, y_r = (torch.zeros(B, H0 * hd, device=DEV) for _ in range(2))
    k.attn(q, H0 * hd, kc, vc, y, pos, B, H0, H0 // n_kv0, hd, S, ml, osc, cnt)
    k.attn_rows(q, H0 * hd, kc, vc, y_r, rows, B, H0, H0 // n_kv0, hd, S,
                ml, osc)
    assert torch.equal(y_r, y) and y.abs().sum() > 0
    z, z_r = _q80_bufs(B, H0, hd), _q80_bufs(B, H0, hd)
    k.attn(q, H0 * hd, kc, vc, y, pos, B, H0, H0 // n_kv0, hd, S, ml, osc, cnt,
           *z)
    k.attn_rows(q, H0 * hd, kc, vc, y_r, rows, B, H0, H0 // n_kv0, hd, S,
                ml, osc, *z_r)
    for a, b in zip(z_r, z):
        assert torch.equal(a, b)


def test_rows_advance(k):
    rows = table([[64, 3], [0, 0], [128, 31], [7, 7]])
    k.rows_advance(rows, 3)
    assert rows.tolist() == [[64, 4], [0, 1], [128, 32], [7, 7]]


# ------------------------------------------------------------- ragged writes

SLOTS, SEQ = 3, 32
RAGGED = [(2, 5), (0, 0), (1, 17), (2, 6)]  # (slot, pos) per row


def _ragged_table():
    return table([[s * SEQ, p] for s, p in RAGGED])


def _check_ragged_writes(kc, vc, want_k, want_v, kv_dt):
    atol = 1e-5 if kv_dt == torch.float32 else 2e-3
    written = [s * SEQ + p for s, p in RAGGED]
    for b, r in enumerate(written):
        assert torch.allclose(kc[r].float().cpu(), want_k[b], atol=atol), b
        assert torch.allclose(vc[r].float().cpu(), want_v[b], atol=atol), b
    untouched = torch.ones(SLOTS * SEQ, dtype=torch.bool)
    untouched[written] = False
    assert not kc.cpu()[untouched].any() and not vc.cpu()[untouched].any()


@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("style", [0, 1])
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_kv_rows_ragged(k, style, kv_dt, hd):
    qh, kvh, B = 4, 2, len(RAGGED)
    q_dim0, kv_dim0 = qh * hd, kvh * hd
    ld = q_dim0 + 2 * kv_dim0
    buf = rand(B, ld, seed=530 + hd)
    src = buf.cpu().clone()
    kc, vc = (torch.zeros(SLOTS * SEQ, kv_dim0, dtype=kv_dt, device=DEV)
              for _ in range(2))
    k.rope_kv_rows(buf, ld, q_dim0, kv_dim0, rope_cache(SEQ, hd),
                   _ragged_table(), kc, vc, hd, style, B)
    rope = R.rope_llama if style == 0 else R.rope_falcon
    rc = R.rope_cache(SEQ, hd, 10000.0)
    positions = torch.tensor([p for _, p in RAGGED])
    want_q = rope(src[:, :q_dim0], rc, positions, hd)
    want_k = rope(src[:, q_dim0: q_dim0 + kv_dim0], rc, positions, hd)
    assert torch.allclose(buf[:, :q_dim0].cpu(), want_q, atol=1e-5)
    _check_ragged_writes(kc, vc, want_k, src[:, q_dim0 + kv_dim0:], kv_dt)


@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_kv_qknorm_rows_ragged(k, kv_dt, hd):
    qh, kvh, B, eps = 4, 2, len(RAGGED), 1e-6
    q_dim0, kv_dim0 = qh * hd, kvh * hd
    ld = q_dim0 + 2 * kv_dim0
    buf = rand(B, ld, seed=540 + hd)
    src = buf.cpu().clone()
    wq = rand(hd, seed=541).abs() + 0.5
    wk = rand(hd, seed=542).abs() + 0.5
    kc, vc = (torch.zeros(SLOTS * SEQ, kv_dim0, dtype=kv_dt, device=DEV)
              for _ in range(2))
    k.rope_kv_qknorm_rows(buf, ld, q_dim0, kv_dim0, rope_cache(SEQ, hd),
                          _ragged_table(), kc, vc, hd, wq, wk, eps, B)
    rc = R.rope_cache(SEQ, hd, 10000.0)
    positions = torch.tensor([p for _, p in RAGGED])

    def norm_rope(x, w):
        n = R.rms_norm(x.reshape(B, -1, hd), w.cpu(), eps).reshape(B, -1)
        return R.rope_falcon(n, rc, positions, hd)

    want_q = norm_rope(src[:, :q_dim0], wq)
    want_k = norm_rope(src[:, q_dim0: q_dim0 + kv_dim0], wk)
    assert torch.allclose(buf[:, :q_dim0].cpu(), want_q, atol=1e-5)
    _check_ragged_writes(kc, vc, want_k, src[:, q_dim0 + kv_dim0:], kv_dt)


# ---------------------------------------------------------- ragged attention

H0, N_KV0, STRIDE = 4, 2, 576
# edges of the 16-lane groups, of one 16*S round (128 at S=8) and of four
# rounds (512 at S=8)
LENGTHS = [1, 15, 16, 17, 128, 129, 515]
ROW_SLOTS = [3, 0, 6, 1, 5, 2, 4]  # slots not in row order


@pytest.fixture(scope="module")
def ragged_attn():
    """Per head_dim: q, f32 K/V caches of 7 slots and R.attention of every
    row on its own slot slice. Computed once, shared, never written."""
    out = {}
    for hd in (64, 128):
        kv_dim0 = N_KV0 * hd
        B = len(LENGTHS)
        kc = rand(B * STRIDE, kv_dim0, seed=550 + hd, scale=0.3)
        vc = rand(B * STRIDE, kv_dim0, seed=551 + hd)
        q = rand(B, H0 * hd, seed=552 + hd)
        kc_c, vc_c, q_c = kc.cpu(), vc.cpu(), q.cpu()
        want = torch.cat([
            R.attention(q_c[b: b + 1], kc_c[s * STRIDE: (s + 1) * STRIDE],
                        vc_c[s * STRIDE: (s + 1) * STRIDE],
                        torch.tensor([n - 1]), H0, hd)
            for b, (s, n) in enumerate(zip(ROW_SLOTS, LENGTHS))])
        out[hd] = (q, kc, vc, want)
    return out


def _ragged_attn_table():
    return table([[s * STRIDE, n - 1] for s, n in zip(ROW_SLOTS, LENGTHS)])


def _run_attn_rows(k, q, kc, vc, hd, S, quant):
    B = len(LENGTHS)
    ml, osc = _attn_bufs(B, H0, hd, S)
    y = torch.zeros(B, H0 * hd, device=DEV)
    z = _q80_bufs(B, H0, hd) if quant else ()
    k.attn_rows(q, H0 * hd, kc, vc, y, _ragged_attn_table(), B, H0,
                H0 // N_KV0, hd, S, ml, osc, *z)
    return z if quant else y


@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("S", [8, 16])
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_rows_ragged(k, ragged_attn, hd, S, kv_dt):
    q, kc, vc, want = ragged_attn[hd]
    kc, vc = kc.to(kv_dt), vc.to(kv_dt)
    atol, rtol = (1e-4, 1e-3) if kv_dt == torch.float32 else (2e-3, 1e-2)
    y = _run_attn_rows(k, q, kc, vc, hd, S, quant=False).cpu()
    err = (y - want).abs().max(dim=1).values
    print(f"attn_rows hd={hd} S={S} {kv_dt}: max err per row {err.tolist()}")
    assert torch.allclose(y, want, atol=atol, rtol=rtol), err
    zq, zs, _ = _run_attn_rows(k, q, kc, vc, hd, S, quant=True)
    deq = R.q80_dequantize(zq.cpu(), zs.cpu())
    qerr = (deq - want).abs().max().item()
    print(f"  Q80 output: max err {qerr}, bound {want.abs().max().item() / 100}")
    assert qerr <= want.abs().max().item() / 100


@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("S", [8, 16])
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_rows_isolation(k, ragged_attn, hd, S, kv_dt):
    """Poisoning every cache row outside each row's own base..base+pos (the
    later rows of its slot, all of its neighbours) changes no output bit:
    fails on a wrong plen or a wrong base."""
    q, kc, vc, _ = ragged_attn[hd]
    kc, vc = kc.to(kv_dt), vc.to(kv_dt)
    own = torch.zeros(kc.shape[0], dtype=torch.bool, device=DEV)
    for s, n in zip(ROW_SLOTS, LENGTHS):
        own[s * STRIDE: s * STRIDE + n] = True
    kc_p, vc_p = kc.clone(), vc.clone()
    kc_p[~own] = 1e4
    vc_p[~own] = 1e4
    y = _run_attn_rows(k, q, kc, vc, hd, S, quant=False)
    y_p = _run_attn_rows(k, q, kc_p, vc_p, hd, S, quant=False)
    assert torch.equal(y_p, y)
    z = _run_attn_rows(k, q, kc, vc, hd, S, quant=True)
    z_p = _run_attn_rows(k, q, kc_p, vc_p, hd, S, quant=True)
    for a, b in zip(z_p, z):
        assert torch.equal(a, b)
