"""Paged forms of the positional kernels (rope_kv_paged, rope_kv_qknorm_paged,
attn_paged): the row-table kernels with every cache row found through a page
table. Only addresses differ, so every comparison is bit for bit: against
the *_rows kernels on the same K/V laid out contiguously."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
KV_DTYPES = [torch.float32, torch.float16]
PAGE_SIZES = [16, 64]


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
    from dllama_amd.ops import reference as R
    return R.rope_cache(seq, hd, 10000.0).to(DEV).reshape(seq, hd).contiguous()


def _attn_bufs(B, H0, hd, S):
    return (torch.zeros(B * H0 * S * 2, device=DEV),
            torch.zeros(B * H0 * S * hd, device=DEV))


def _q80_bufs(B, H0, hd):
    nb = H0 * hd // 32
    return (torch.zeros(B, H0 * hd, dtype=torch.int8, device=DEV),
            torch.zeros(B, nb, device=DEV), torch.zeros(B, nb, device=DEV))


def page_map(n_slots, pps, spare, seed):
    """int64 [n_slots, pps] on the host: a seeded permutation of
    n_slots*pps + spare page ids, the spare ones left unmapped. seed None:
    the identity."""
    n = n_slots * pps
    if seed is None:
        return torch.arange(n).reshape(n_slots, pps), n
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n + spare, generator=g)
    return perm[:n].reshape(n_slots, pps), n + spare


def pool_rows(pmap, P, stride):
    """For a contiguous cache of n_slots*stride rows (stride = pps*P): the
    pool row of every contiguous row, int64 on the device."""
    n_slots, pps = pmap.shape
    assert stride == pps * P
    t = torch.arange(stride)
    rows = pmap[:, t // P] * P + t % P   # [n_slots, stride]
    return rows.reshape(-1).to(DEV)


def scatter(cache, rows, n_pool_rows, fill=0.0):
    pool = torch.full((n_pool_rows, cache.shape[1]), fill, dtype=cache.dtype,
                      device=DEV)
    pool[rows] = cache
    return pool


# ---------------------------------------------------------- ragged attention

H0, N_KV0, STRIDE = 4, 2, 576
# the ragged case of tests/test_rows_ops.py: edges of the 16-lane groups, of
# one 16*S round and of four rounds; 576 = 36 pages of 16 = 9 of 64
LENGTHS = [1, 15, 16, 17, 128, 129, 515]
ROW_SLOTS = [3, 0, 6, 1, 5, 2, 4]
N_SLOTS = len(LENGTHS)


@pytest.fixture(scope="module")
def ragged():
    """Per head_dim: q and f32 K/V caches of 7 contiguous slots. Computed
    once, shared, never written."""
    out = {}
    for hd in (64, 128):
        kv_dim0 = N_KV0 * hd
        kc = rand(N_SLOTS * STRIDE, kv_dim0, seed=550 + hd, scale=0.3)
        vc = rand(N_SLOTS * STRIDE, kv_dim0, seed=551 + hd)
        q = rand(N_SLOTS, H0 * hd, seed=552 + hd)
        out[hd] = (q, kc, vc)
    return out


def _run_rows(k, q, kc, vc, hd, S, quant):
    B = len(LENGTHS)
    ml, osc = _attn_bufs(B, H0, hd, S)
    y = torch.zeros(B, H0 * hd, device=DEV)
    z = _q80_bufs(B, H0, hd) if quant else ()
    rows = table([[s * STRIDE, n - 1] for s, n in zip(ROW_SLOTS, LENGTHS)])
    k.attn_rows(q, H0 * hd, kc, vc, y, rows, B, H0, H0 // N_KV0, hd, S,
                ml, osc, *z)
    return z if quant else (y,)


def _run_paged(k, q, kc, vc, pt, P, hd, S, quant, row_slots=ROW_SLOTS):
    B = len(LENGTHS)
    ml, osc = _attn_bufs(B, H0, hd, S)
    y = torch.zeros(B, H0 * hd, device=DEV)
    z = _q80_bufs(B, H0, hd) if quant else ()
    pps = pt.shape[1]
    rows = table([[s * pps, n - 1] for s, n in zip(row_slots, LENGTHS)])
    k.attn_paged(q, H0 * hd, kc, vc, y, rows, pt, P, B, H0, H0 // N_KV0, hd,
                 S, ml, osc, *z)
    return z if quant else (y,)


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("P", PAGE_SIZES)
@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("S", [8, 16])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("seed", [None, 77], ids=["identity", "scrambled"])
def test_attn_paged_equals_attn_rows(k, ragged, hd, S, kv_dt, P, seed):
    """Identity map: the pool is the contiguous cache. Scrambled: the pages
    are scattered through a seeded permutation with spare pages between."""
    q, kc, vc = ragged[hd]
    kc, vc = kc.to(kv_dt), vc.to(kv_dt)
    pmap, n_pages = page_map(N_SLOTS, STRIDE // P, spare=5, seed=seed)
    rows = pool_rows(pmap, P, STRIDE)
    kp, vp = scatter(kc, rows, n_pages * P), scatter(vc, rows, n_pages * P)
    if seed is None:
        assert torch.equal(kp, kc)
    pt = pmap.to(torch.int32).to(DEV)
    for quant in (False, True):
        want = _run_rows(k, q, kc, vc, hd, S, quant)
        got = _run_paged(k, q, kp, vp, pt, P, hd, S, quant)
        _same(got, want)
        assert want[0].abs().sum() > 0


@pytest.mark.parametrize("P", PAGE_SIZES)
@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("S", [8, 16])
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_paged_isolation(k, ragged, hd, S, kv_dt, P):
    """Poisoning every pool row outside each row's own pages below its
    length (the rest of its last page, its later pages, every neighbour and
    spare page) changes no output bit."""
    q, kc, vc = ragged[hd]
    kc, vc = kc.to(kv_dt), vc.to(kv_dt)
    pmap, n_pages = page_map(N_SLOTS, STRIDE // P, spare=5, seed=78)
    rows = pool_rows(pmap, P, STRIDE)
    kp, vp = scatter(kc, rows, n_pages * P), scatter(vc, rows, n_pages * P)
    own = torch.zeros(n_pages * P, dtype=torch.bool, device=DEV)
    for s, n in zip(ROW_SLOTS, LENGTHS):
        own[rows[s * STRIDE: s * STRIDE + n]] = True
    assert int(own.sum()) == sum(LENGTHS)
    kp_p, vp_p = kp.clone(), vp.clone()
    kp_p[~own] = 1e4
    vp_p[~own] = 1e4
    pt = pmap.to(torch.int32).to(DEV)
    for quant in (False, True):
        clean = _run_paged(k, q, kp, vp, pt, P, hd, S, quant)
        dirty = _run_paged(k, q, kp_p, vp_p, pt, P, hd, S, quant)
        _same(dirty, clean)


@pytest.mark.parametrize("P", PAGE_SIZES)
@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("S", [8, 16])
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_paged_shared_pages(k, ragged, hd, S, kv_dt, P):
    """The slots of the 129- and the 515-row sequences hold the same first
    128 positions. With both tables naming one set of physical pages for
    them, the bits are those of the private copies."""
    q, kc, vc = ragged[hd]
    kc, vc = kc.to(kv_dt).clone(), vc.to(kv_dt).clone()
    a, b = ROW_SLOTS[5], ROW_SLOTS[6]   # lengths 129 and 515
    kc[b * STRIDE: b * STRIDE + 128] = kc[a * STRIDE: a * STRIDE + 128]
    vc[b * STRIDE: b * STRIDE + 128] = vc[a * STRIDE: a * STRIDE + 128]
    pmap, n_pages = page_map(N_SLOTS, STRIDE // P, spare=5, seed=79)
    rows = pool_rows(pmap, P, STRIDE)
    kp, vp = scatter(kc, rows, n_pages * P), scatter(vc, rows, n_pages * P)
    shared = pmap.clone()
    private = shared[b, : 128 // P].clone()
    shared[b, : 128 // P] = shared[a, : 128 // P]
    # b's own copies of the prefix are not read any more: poison them
    for page in private.tolist():
        kp[page * P: (page + 1) * P] = 1e4
        vp[page * P: (page + 1) * P] = 1e4
    pt = shared.to(torch.int32).to(DEV)
    for quant in (False, True):
        want = _run_rows(k, q, kc, vc, hd, S, quant)
        got = _run_paged(k, q, kp, vp, pt, P, hd, S, quant)
        _same(got, want)


# ------------------------------------------------------------- rope + write

SLOTS, SEQ = 4, 64
# (slot, pos): positions 0, 15, 16, 17 (page edges at P=16), and two rows of
# one slot (a prompt chunk)
RAGGED = [(2, 0), (0, 15), (1, 16), (3, 17), (3, 18)]


def _rope_case(k, kv_dt, hd, P, seed, qknorm, style=1):
    qh, kvh, B = 4, 2, len(RAGGED)
    q_dim0, kv_dim0 = qh * hd, kvh * hd
    ld = q_dim0 + 2 * kv_dim0
    buf = rand(B, ld, seed=600 + hd)
    buf_p = buf.clone()
    cache = rope_cache(SEQ, hd)
    wq = rand(hd, seed=601).abs() + 0.5
    wk = rand(hd, seed=602).abs() + 0.5
    pps = SEQ // P
    pmap, n_pages = page_map(SLOTS, pps, spare=3, seed=seed)
    kc, vc = (torch.zeros(SLOTS * SEQ, kv_dim0, dtype=kv_dt, device=DEV)
              for _ in range(2))
    kp, vp = (torch.zeros(n_pages * P, kv_dim0, dtype=kv_dt, device=DEV)
              for _ in range(2))
    rows = table([[s * SEQ, p] for s, p in RAGGED])
    rows_p = table([[s * pps, p] for s, p in RAGGED])
    pt = pmap.to(torch.int32).to(DEV)
    if qknorm:
        k.rope_kv_qknorm_rows(buf, ld, q_dim0, kv_dim0, cache, rows, kc, vc,
                              hd, wq, wk, 1e-6, B)
        k.rope_kv_qknorm_paged(buf_p, ld, q_dim0, kv_dim0, cache, rows_p, pt,
                               P, kp, vp, hd, wq, wk, 1e-6, B)
    else:
        k.rope_kv_rows(buf, ld, q_dim0, kv_dim0, cache, rows, kc, vc, hd,
                       style, B)
        k.rope_kv_paged(buf_p, ld, q_dim0, kv_dim0, cache, rows_p, pt, P,
                        kp, vp, hd, style, B)
    assert torch.equal(buf_p, buf)      # q rotated in place, the same
    written = [s * SEQ + p for s, p in RAGGED]
    assert kc[written].abs().sum() > 0 and vc[written].abs().sum() > 0
    if seed is None:
        assert torch.equal(kp, kc) and torch.equal(vp, vc)
    # the pool gathered back through the map is the contiguous cache ...
    back = pool_rows(pmap, P, SEQ)
    assert torch.equal(kp[back], kc) and torch.equal(vp[back], vc)
    # ... and every pool row the map does not name for a written position
    # is still zero
    untouched = torch.ones(n_pages * P, dtype=torch.bool, device=DEV)
    untouched[back[written]] = False
    assert not kp[untouched].any() and not vp[untouched].any()


@pytest.mark.parametrize("P", PAGE_SIZES)
@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("style", [0, 1])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("seed", [None, 80], ids=["identity", "scrambled"])
def test_rope_kv_paged(k, style, kv_dt, hd, P, seed):
    _rope_case(k, kv_dt, hd, P, seed, qknorm=False, style=style)


@pytest.mark.parametrize("P", PAGE_SIZES)
@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("seed", [None, 81], ids=["identity", "scrambled"])
def test_rope_kv_qknorm_paged(k, kv_dt, hd, P, seed):
    _rope_case(k, kv_dt, hd, P, seed, qknorm=True)


def test_paged_host_checks(k):
    """What the bindings refuse before any launch."""
    hd, B, S, P = 64, 2, 8, 16
    kv_dim0 = N_KV0 * hd
    q = rand(B, H0 * hd, seed=1)
    kc, vc = (torch.zeros(4 * P, kv_dim0, dtype=torch.float16, device=DEV)
              for _ in range(2))
    y = torch.zeros(B, H0 * hd, device=DEV)
    ml, osc = _attn_bufs(B, H0, hd, S)
    rows = table([[0, 3], [2, 5]])
    pt = table([[0, 1], [2, 3]])

    def run(rows=rows, pt=pt, P=P, kc=kc, vc=vc):
        k.attn_paged(q, H0 * hd, kc, vc, y, rows, pt, P, B, H0, H0 // N_KV0,
                     hd, S, ml, osc)

    run()
    for bad in (2, 48, 512):
        with pytest.raises(RuntimeError, match="page_size"):
            run(P=bad)
    with pytest.raises(RuntimeError, match="whole pages"):
        run(kc=kc[: 4 * P - 1], vc=vc[: 4 * P - 1])
    with pytest.raises(RuntimeError, match="page table"):
        run(pt=pt.to(torch.int64))
    with pytest.raises(RuntimeError, match="page table"):
        run(pt=pt.t())          # not contiguous
    with pytest.raises(RuntimeError, match="GPU tensor|page table"):
        run(pt=pt.cpu())
    with pytest.raises(RuntimeError, match="row table"):
        run(rows=rows[:1])      # fewer table rows than batch
