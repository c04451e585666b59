"""The positional kernels on a Q80 KV cache (int8 code plane + f16 scale
plane per K and V), through all nine bindings.

Write side, per block of 32 cache elements with d = f32(scale) and `want`
the CPU reference (R.rope_* / R.rms_norm, V as it is):
  |code*d - want| <= 0.5*d + 1e-4 + 1e-3*|want|   the quantiser's half step
                                                  plus the f32 tolerance; the
                                                  f16 rounding of d moves
                                                  code*d by |want| * 2^-11
  d == f16(max|want_block| / 127)                 rtol 1e-3, atol 1e-6
No element is exempt. q is the f16 binding's q bit for bit and no cache row
but the addressed ones changes.

Read side: the caches are built with the reference quantiser and `want` is
R.attention over the dequantised values, which are exactly what the kernels
read; the tolerances are those of tests/test_attn_wide.py (wide kernel) and
tests/test_rows_ops.py (split + combine) for the f16 cache."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd.ops import reference as R

from test_attn_wide import (POSITIONS, ROW_POS, ROW_SLOTS, SEQ, SHAPES,
                            STRIDE, check_q80, paged_pool, q80_bufs, rand,
                            same, table)

DEV = "cuda"


@pytest.fixture(scope="module")
def k():
    from dllama_amd.ops import hip_ops
    return hip_ops()


def rope_cache(seq, hd):
    return R.rope_cache(seq, hd, 10000.0).to(DEV).reshape(seq, hd).contiguous()


# ================================================================ write side

W_POS = (0, 5, 37)
W_SLOTS = (2, 0, 1)  # slots not in row order
W_SEQ = 40           # cache rows per slot
W_P = 4              # page size of the paged form
CODE0, SCALE0 = 77, 3.0  # what every cache row holds before the launch


def w_page_table():
    """Three slots of W_SEQ/W_P pages in a pool with spare pages, through a
    seeded permutation."""
    pps = W_SEQ // W_P
    g = torch.Generator().manual_seed(811)
    ids = torch.randperm(3 * pps + 5, generator=g)[: 3 * pps].reshape(3, pps)
    return ids.to(torch.int32)


def w_rows_of(addressing):
    """(cache rows in the pool, rows written per batch row)."""
    if addressing == "seq":
        return W_SEQ, list(W_POS)
    if addressing == "rows":
        return 3 * W_SEQ, [s * W_SEQ + p for s, p in zip(W_SLOTS, W_POS)]
    pt = w_page_table()
    return (3 * (W_SEQ // W_P) + 5) * W_P, [
        int(pt[s, p // W_P]) * W_P + p % W_P for s, p in zip(W_SLOTS, W_POS)]


def w_launch(k, name, addressing, buf, dims, cache, planes, tail):
    """One write of the three rows. seq: the single-sequence binding places
    row b at pos+b, so the three positions are three one-row launches."""
    ld, q_dim0, kv_dim0 = dims
    kc, vc, kw = planes
    if addressing == "seq":
        for b, p in enumerate(W_POS):
            getattr(k, name)(buf[b: b + 1], ld, q_dim0, kv_dim0, cache,
                             table([p]), kc, vc, *tail, 1, **kw)
    elif addressing == "rows":
        rows = table([[s * W_SEQ, p] for s, p in zip(W_SLOTS, W_POS)])
        getattr(k, name + "_rows")(buf, ld, q_dim0, kv_dim0, cache, rows, kc,
                                   vc, *tail, 3, **kw)
    else:
        pps = W_SEQ // W_P
        rows = table([[s * pps, p] for s, p in zip(W_SLOTS, W_POS)])
        getattr(k, name + "_paged")(buf, ld, q_dim0, kv_dim0, cache, rows,
                                    w_page_table().to(DEV), W_P, kc, vc,
                                    *tail, 3, **kw)


def check_blocks(codes, scales, want, what):
    """codes int8 [B, n], scales f16 [B, n/32], want f32 [B, n]."""
    B, n = want.shape
    wb = want.reshape(B, n // 32, 32)
    c = codes.reshape(B, n // 32, 32).float()
    d = scales.float().unsqueeze(-1)
    err = (c * d - wb).abs()
    bound = 0.5 * d + 1e-4 + 1e-3 * wb.abs()
    d_want = (wb.abs().amax(dim=-1) / 127).to(torch.float16).float()
    print(f"{what}: max err {err.max().item():.3e}, least slack "
          f"{(bound - err).min().item():.3e}, max |d - d_want| "
          f"{(scales.float() - d_want).abs().max().item():.3e}")
    assert (err <= bound).all(), what
    assert torch.allclose(scales.float(), d_want, rtol=1e-3, atol=1e-6), what


@pytest.mark.parametrize("addressing", ["seq", "rows", "paged"])
@pytest.mark.parametrize("form", ["llama", "neox", "qknorm"])
@pytest.mark.parametrize("shape", SHAPES)
def test_write_q80(k, shape, form, addressing):
    hd, qh, kvh = shape
    q_dim0, kv_dim0 = qh * hd, kvh * hd
    ld = q_dim0 + 2 * kv_dim0
    dims = (ld, q_dim0, kv_dim0)
    buf = rand(3, ld, seed=800 + hd)
    src = buf.cpu().clone()
    cache = rope_cache(W_SEQ, hd)
    eps = 1e-6
    wq = rand(hd, seed=801).abs() + 0.5
    wk = rand(hd, seed=802).abs() + 0.5
    if form == "qknorm":
        name, tail = "rope_kv_qknorm", (hd, wq, wk, eps)
    else:
        name, tail = "rope_kv", (hd, 0 if form == "llama" else 1)
    n_rows, written = w_rows_of(addressing)
    kc = torch.full((n_rows, kv_dim0), CODE0, dtype=torch.int8, device=DEV)
    vc = kc.clone()
    ks = torch.full((n_rows, kv_dim0 // 32), SCALE0, dtype=torch.float16,
                    device=DEV)
    vs = ks.clone()
    w_launch(k, name, addressing, buf, dims, cache,
             (kc, vc, {"k_scales": ks, "v_scales": vs}), tail)

    # the f16 binding on the same input: q bit for bit
    buf16 = src.to(DEV)
    kc16 = torch.zeros(n_rows, kv_dim0, dtype=torch.float16, device=DEV)
    w_launch(k, name, addressing, buf16, dims, cache,
             (kc16, torch.zeros_like(kc16), {}), tail)
    qdiff = (buf[:, :q_dim0] != buf16[:, :q_dim0]).nonzero().tolist()
    print(f"{form} {addressing} shape={shape}: {len(qdiff)} q elements "
          f"differ from the f16 binding's, max "
          f"{(buf[:, :q_dim0] - buf16[:, :q_dim0]).abs().max().item():.3e}, "
          f"first {qdiff[:6]}")
    assert torch.equal(buf[:, :q_dim0], buf16[:, :q_dim0])
    assert not torch.equal(buf[:, :q_dim0].cpu(), src[:, :q_dim0])
    # k and v of the input buffer are read, not written
    assert torch.equal(buf[:, q_dim0:].cpu(), src[:, q_dim0:])

    rc = R.rope_cache(W_SEQ, hd, 10000.0)
    positions = torch.tensor(W_POS)
    want_k = src[:, q_dim0: q_dim0 + kv_dim0]
    if form == "qknorm":
        want_k = R.rms_norm(want_k.reshape(3, -1, hd), wk.cpu(),
                            eps).reshape(3, -1)
    rope = R.rope_llama if form == "llama" else R.rope_falcon
    want_k = rope(want_k, rc, positions, hd)
    want_v = src[:, q_dim0 + kv_dim0:]
    what = f"{form} {addressing} shape={shape}"
    check_blocks(kc.cpu()[written], ks.cpu()[written], want_k, what + " K")
    check_blocks(vc.cpu()[written], vs.cpu()[written], want_v, what + " V")
    # no cache row but the three addressed ones changed
    assert len(set(written)) == 3
    untouched = torch.ones(n_rows, dtype=torch.bool)
    untouched[written] = False
    for codes, scales in ((kc, ks), (vc, vs)):
        assert (codes.cpu()[untouched] == CODE0).all(), what
        assert (scales.cpu()[untouched] == SCALE0).all(), what


def test_write_q80_zero_block(k):
    """An all-zero V block stores code 0 and scale 0 (no 0/0)."""
    hd, qh, kvh = 64, 2, 1
    q_dim0, kv_dim0 = qh * hd, kvh * hd
    ld = q_dim0 + 2 * kv_dim0
    buf = rand(1, ld, seed=820)
    buf[0, q_dim0 + kv_dim0: q_dim0 + kv_dim0 + 32] = 0.0
    kc = torch.full((4, kv_dim0), CODE0, dtype=torch.int8, device=DEV)
    vc = kc.clone()
    ks = torch.full((4, kv_dim0 // 32), SCALE0, dtype=torch.float16,
                    device=DEV)
    vs = ks.clone()
    k.rope_kv(buf, ld, q_dim0, kv_dim0, rope_cache(4, hd), table([2]), kc, vc,
              hd, 0, 1, k_scales=ks, v_scales=vs)
    assert not vc[2, :32].any() and vs[2, 0].item() == 0.0
    assert vs[2, 1].item() > 0.0 and torch.isfinite(vs.float()).all()


# ================================================================= read side

def q80_cache(x):
    """f32 [rows, n] -> (codes, scales) on the device, dequantised on the
    CPU: the values the kernels read."""
    q, s = R.q80_quantize_f16(x.cpu())
    return q.to(DEV), s.to(DEV), R.q80_dequantize(q, s.float())


@functools.lru_cache(maxsize=None)
def seq_case(shape):
    """q of two rows and the Q80 caches of one sequence. Computed once per
    shape, never written."""
    hd, H0, n_kv0 = shape
    kq, ks, kd = q80_cache(rand(SEQ, n_kv0 * hd, seed=830 + hd, scale=0.3))
    vq, vs, vd = q80_cache(rand(SEQ, n_kv0 * hd, seed=831 + hd))
    q = rand(2, H0 * hd, seed=832 + hd)
    return q, (kq, vq, ks, vs), (kd, vd)


@functools.lru_cache(maxsize=None)
def seq_want(shape, pos):
    hd, H0, _ = shape
    q, _, (kd, vd) = seq_case(shape)
    return R.attention(q.cpu(), kd, vd, torch.tensor([pos, pos + 1]), H0, hd)


def split_scratch(B, H0, hd, S):
    return (torch.zeros(B * H0 * S * 2, device=DEV),
            torch.zeros(B * H0 * S * hd, device=DEV),
            torch.zeros(B * H0, dtype=torch.int32, device=DEV))


def run_seq(k, shape, pos_t, B, S, quant):
    hd, H0, n_kv0 = shape
    q, (kq, vq, ks, vs), _ = seq_case(shape)
    y = torch.zeros(B, H0 * hd, device=DEV)
    z = q80_bufs(B, H0, hd) if quant else ()
    k.attn(q, H0 * hd, kq, vq, y, pos_t, B, H0, H0 // n_kv0, hd, S,
           *split_scratch(B, H0, hd, S), *z, k_scales=ks, v_scales=vs)
    return z if quant else y


# (splits, Q80 triple out): the wide kernel, split + combine to the triple
# at both split counts, split + combine to f32
READ_MODES = [(1, True), (8, True), (16, True), (8, False)]


def check_read(got, want, S, quant, what):
    if S == 1:
        check_q80(got, want, what)  # tests/test_attn_wide.py
        return
    if quant:                       # tests/test_rows_ops.py, f16 cache
        zq, zs, _ = got
        qerr = (R.q80_dequantize(zq.cpu(), zs.cpu()) - want).abs().max().item()
        print(f"{what}: Q80 output max err {qerr:.3e}, bound "
              f"{want.abs().max().item() / 100:.3e}")
        assert qerr <= want.abs().max().item() / 100, what
        return
    y = got.cpu()
    print(f"{what}: max err {(y - want).abs().max().item():.3e}")
    assert torch.allclose(y, want, atol=2e-3, rtol=1e-2), what


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("S,quant", READ_MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_q80_matches_reference(k, shape, S, quant, B, pos):
    """Row b attends to positions 0..pos+b."""
    got = run_seq(k, shape, table([pos]), B, S, quant)
    check_read(got, seq_want(shape, pos)[:B], S, quant,
               f"shape={shape} S={S} quant={quant} B={B} pos={pos}")


# --------------------------------------------------------------- row table

@functools.lru_cache(maxsize=None)
def rows_case(shape):
    """q of three rows, the Q80 slot caches and R.attention of every row
    over its own slot. Computed once per shape, never written."""
    hd, H0, n_kv0 = shape
    kq, ks, kd = q80_cache(rand(3 * STRIDE, n_kv0 * hd, seed=840 + hd,
                                scale=0.3))
    vq, vs, vd = q80_cache(rand(3 * STRIDE, n_kv0 * hd, seed=841 + hd))
    q = rand(3, H0 * hd, seed=842 + hd)
    want = torch.cat([
        R.attention(q[b: b + 1].cpu(), kd[s * STRIDE: (s + 1) * STRIDE],
                    vd[s * STRIDE: (s + 1) * STRIDE], torch.tensor([p]),
                    H0, hd)
        for b, (s, p) in enumerate(zip(ROW_SLOTS, ROW_POS))])
    return q, (kq, vq, ks, vs), want


def run_rows(k, shape, q, planes, S):
    hd, H0, n_kv0 = shape
    kq, vq, ks, vs = planes
    z = q80_bufs(3, H0, hd)
    ml, osc, _ = split_scratch(3, H0, hd, S)
    k.attn_rows(q, H0 * hd, kq, vq, torch.zeros(3, H0 * hd, device=DEV),
                table([[s * STRIDE, p] for s, p in zip(ROW_SLOTS, ROW_POS)]),
                3, H0, H0 // n_kv0, hd, S, ml, osc, *z, k_scales=ks,
                v_scales=vs)
    return z


@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_q80_rows_isolation(k, shape, S):
    """Every row has its own length and base: the outputs match the
    reference, and no bit changes with what the code and scale rows outside
    each row's own base..base+pos hold."""
    q, planes, want = rows_case(shape)
    own = torch.zeros(planes[0].shape[0], dtype=torch.bool, device=DEV)
    for s, p in zip(ROW_SLOTS, ROW_POS):
        own[s * STRIDE: s * STRIDE + p + 1] = True
    z = run_rows(k, shape, q, planes, S)
    check_read(z, want, S, True, f"rows shape={shape} S={S}")
    for code in (127, -127):
        kq, vq, ks, vs = (t.clone() for t in planes)
        kq[~own] = code
        vq[~own] = code
        ks[~own] = 6e4
        vs[~own] = 6e4
        same(run_rows(k, shape, q, (kq, vq, ks, vs), S), z)


# ------------------------------------------------------------------- paged

@pytest.mark.parametrize("P,share", [(4, False), (8, False), (64, False),
                                     (8, True)])
@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_q80_paged_equals_rows(k, shape, S, P, share):
    """Only the addressing differs from the row table, so the bits are the
    same; with share, two rows read their first 128 positions from one set
    of physical pages."""
    hd, H0, n_kv0 = shape
    q, planes, _ = rows_case(shape)
    if share:
        planes = tuple(t.clone() for t in planes)
        a, b = ROW_SLOTS[1], ROW_SLOTS[2]
        for t in planes:
            t[b * STRIDE: b * STRIDE + 128] = t[a * STRIDE: a * STRIDE + 128]
    want = run_rows(k, shape, q, planes, S)
    kq, vq, ks, vs = planes
    kqp, vqp, pt = paged_pool(kq, vq, P, share)
    ksp, vsp, pt2 = paged_pool(ks, vs, P, share)
    assert torch.equal(pt, pt2)
    z = q80_bufs(3, H0, hd)
    ml, osc, _ = split_scratch(3, H0, hd, S)
    rows = table([[s * (STRIDE // P), p] for s, p in zip(ROW_SLOTS, ROW_POS)])
    k.attn_paged(q, H0 * hd, kqp, vqp, torch.zeros(3, H0 * hd, device=DEV),
                 rows, pt, P, 3, H0, H0 // n_kv0, hd, S, ml, osc, *z,
                 k_scales=ksp, v_scales=vsp)
    same(z, want)


# ----------------------------------------------------------- graph capture

@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_q80_graph_replay(k, shape, S):
    """A launch captured at pos 10 replays correctly at any position."""
    hd, H0, n_kv0 = shape
    q, (kq, vq, ks, vs), _ = seq_case(shape)
    pos_t = table([10])
    z = q80_bufs(1, H0, hd)
    y = torch.zeros(1, H0 * hd, device=DEV)
    sc = split_scratch(1, H0, hd, S)

    def launch():
        k.attn(q, H0 * hd, kq, vq, y, pos_t, 1, H0, H0 // n_kv0, hd, S, *sc,
               *z, k_scales=ks, v_scales=vs)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for pos in (10, 200, 300):
        pos_t.fill_(pos)
        g.replay()
        got = [t.clone() for t in z]
        same(got, run_seq(k, shape, table([pos]), 1, S, True))


# ---------------------------------------------------------------- refusals

def test_q80_refusals(k):
    hd, H0, n_kv0 = 64, 2, 1
    kv_dim0 = n_kv0 * hd
    seq = 8
    kc = torch.zeros(seq, kv_dim0, dtype=torch.int8, device=DEV)
    vc = torch.zeros_like(kc)
    ks = torch.zeros(seq, kv_dim0 // 32, dtype=torch.float16, device=DEV)
    vs = torch.zeros_like(ks)
    q = rand(1, H0 * hd + 2 * kv_dim0, seed=850)
    y = torch.zeros(1, H0 * hd, device=DEV)
    pos = table([0])
    sc = split_scratch(1, H0, hd, 8)

    def attn(**kw):
        k.attn(q, H0 * hd + 2 * kv_dim0, kc, vc, y, pos, 1, H0, H0 // n_kv0,
               hd, 8, *sc, **kw)

    def rope_kv(**kw):
        k.rope_kv(q, H0 * hd + 2 * kv_dim0, H0 * hd, kv_dim0,
                  rope_cache(seq, hd), pos, kc, vc, hd, 0, 1, **kw)

    def rope_kv_qknorm(**kw):
        w = torch.ones(hd, device=DEV)
        k.rope_kv_qknorm(q, H0 * hd + 2 * kv_dim0, H0 * hd, kv_dim0,
                         rope_cache(seq, hd), pos, kc, vc, hd, w, w, 1e-6, 1,
                         **kw)

    for call in (attn, rope_kv, rope_kv_qknorm):
        with pytest.raises(RuntimeError, match="k_scales"):
            call()
        with pytest.raises(RuntimeError, match="k_scales"):
            call(k_scales=ks)
        with pytest.raises(RuntimeError, match="float16"):
            call(k_scales=ks.float(), v_scales=vs.float())
        with pytest.raises(RuntimeError, match=r"\[rows, kv_dim0/32\]"):
            call(k_scales=ks[:-1], v_scales=vs[:-1])
        with pytest.raises(RuntimeError, match=r"\[rows, kv_dim0/32\]"):
            call(k_scales=torch.zeros(seq, kv_dim0 // 16, dtype=torch.float16,
                                      device=DEV), v_scales=vs)
        with pytest.raises(RuntimeError, match="contiguous"):
            wide = torch.zeros(seq, kv_dim0 // 16, dtype=torch.float16,
                               device=DEV)
            call(k_scales=wide[:, ::2], v_scales=vs)
        with pytest.raises(RuntimeError, match="device"):
            call(k_scales=ks.cpu(), v_scales=vs)
        call(k_scales=ks, v_scales=vs)  # and the right planes are taken
    # scales without an int8 cache
    kc16 = torch.zeros(seq, kv_dim0, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="int8"):
        k.rope_kv(q, H0 * hd + 2 * kv_dim0, H0 * hd, kv_dim0,
                  rope_cache(seq, hd), pos, kc16, kc16.clone(), hd, 0, 1,
                  k_scales=ks, v_scales=vs)
    # the bindings with no Q80 form
    kv = rand(1, kv_dim0, seed=851)
    with pytest.raises(RuntimeError, match="Q80"):
        k.kv_append(kv, kv, kc, vc, pos)
    d, n = H0 * hd + 2 * kv_dim0, 64
    qs = torch.zeros(d, n // 2, dtype=torch.uint8, device=DEV)
    scales = torch.zeros(d, n // 32, dtype=torch.float16, device=DEV)
    xq = torch.zeros(1, n, dtype=torch.int8, device=DEV)
    xs = torch.zeros(1, n // 32, device=DEV)
    out = torch.zeros(1, d, device=DEV)
    with pytest.raises(RuntimeError, match="Q80"):
        k.q40_gemv_rope(qs, scales, xq, xs, xs.clone(), out, 1,
                        rope_cache(seq, hd), pos, kc, vc, H0 * hd, kv_dim0, hd)
    torch.cuda.synchronize()
