"""The wide single-launch attention (splits=1 with Q80 output) through its
three bindings: against R.attention on the CPU over the K/V values the
kernel reads, then row-table isolation, paged addressing bit for bit against
the row table, and graph replay bit for bit against eager calls.

Per Q80 block of 32 outputs, with d = zs[block] and `want` the reference:
  |zq*d - want| <= 0.5*d + 1e-4 + 1e-3*|want|   the quantiser's half step plus
                                                the f32 attention tolerance
  d == max|want_block| / 127                    rtol 1e-3, atol 1e-6
  zbs[block] == sum of the block's codes        exactly: 32 int8 values sum
                                                exactly in f32
No element is exempt."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd.ops import reference as R

DEV = "cuda"
KV_DTYPES = [torch.float32, torch.float16]
SHAPES = [(128, 4, 2), (64, 2, 1)]  # (head_dim, n_heads0, n_kv_heads0)
# one valid timestep; the group-of-4, wave (16) and round (256) boundaries;
# three rounds
POSITIONS = [0, 3, 4, 15, 16, 254, 255, 256, 599]
SEQ = 608


@pytest.fixture(scope="module")
def k():
    from dllama_amd.ops import hip_ops
    return hip_ops()


def rand(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g) * scale


def table(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


def q80_bufs(B, H0, hd):
    nb = H0 * hd // 32
    return (torch.zeros(B, H0 * hd, dtype=torch.int8, device=DEV),
            torch.zeros(B, nb, device=DEV), torch.zeros(B, nb, device=DEV))


def scratch(B, H0, hd):
    """The split scratch and counter of the bindings, sized for S=1; the
    wide kernel uses none of them."""
    return (torch.zeros(B * H0 * 2, device=DEV),
            torch.zeros(B * H0 * hd, device=DEV),
            torch.zeros(B * H0, dtype=torch.int32, device=DEV))


def check_q80(z, want, what):
    zq, zs, zbs = (t.cpu() for t in z)
    B, n = want.shape
    wb = want.reshape(B, n // 32, 32)
    codes = zq.reshape(B, n // 32, 32).float()
    d = zs.unsqueeze(-1)
    err = (codes * d - wb).abs()
    bound = 0.5 * d + 1e-4 + 1e-3 * wb.abs()
    d_want = wb.abs().amax(dim=-1) / 127
    print(f"{what}: max err {err.max().item():.3e}, least slack "
          f"{(bound - err).min().item():.3e}, max |d - d_want| "
          f"{(zs - d_want).abs().max().item():.3e}")
    assert (err <= bound).all(), what
    assert torch.allclose(zs, d_want, rtol=1e-3, atol=1e-6), what
    assert torch.equal(zbs, codes.sum(dim=-1)), what


# ------------------------------------------------------------ one sequence

@functools.lru_cache(maxsize=None)
def seq_case(shape, kv_dt):
    """q of two rows and the K/V caches of one sequence, in the dtype the
    kernel reads. Computed once per (shape, dtype), never written."""
    hd, H0, n_kv0 = shape
    kc = rand(SEQ, n_kv0 * hd, seed=700 + hd, scale=0.3).to(kv_dt)
    vc = rand(SEQ, n_kv0 * hd, seed=701 + hd).to(kv_dt)
    q = rand(2, H0 * hd, seed=702 + hd)
    return q, kc, vc


@functools.lru_cache(maxsize=None)
def seq_want(shape, kv_dt, pos):
    """R.attention of rows at pos and pos+1, over the caches cast to float."""
    hd, H0, _ = shape
    q, kc, vc = seq_case(shape, kv_dt)
    return R.attention(q.cpu(), kc.cpu().float(), vc.cpu().float(),
                       torch.tensor([pos, pos + 1]), H0, hd)


def run_seq(k, shape, kv_dt, pos_t, B):
    hd, H0, n_kv0 = shape
    q, kc, vc = seq_case(shape, kv_dt)
    z = q80_bufs(B, H0, hd)
    k.attn(q, H0 * hd, kc, vc, torch.zeros(B, H0 * hd, device=DEV), pos_t, B,
           H0, H0 // n_kv0, hd, 1, *scratch(B, H0, hd), *z)
    return z


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_wide_matches_reference(k, shape, kv_dt, B, pos):
    """Row b attends to positions 0..pos+b."""
    z = run_seq(k, shape, kv_dt, table([pos]), B)
    check_q80(z, seq_want(shape, kv_dt, pos)[:B],
              f"shape={shape} {kv_dt} B={B} pos={pos}")


# --------------------------------------------------------------- row table

ROW_POS = (0, 255, 300)
ROW_SLOTS = (2, 0, 1)  # slots not in row order
STRIDE = 320           # cache rows per slot, a multiple of every page size


@functools.lru_cache(maxsize=None)
def rows_case(shape, kv_dt):
    """q of three rows, the slot caches and R.attention of every row over
    its own slot. Computed once per (shape, dtype), never written."""
    hd, H0, n_kv0 = shape
    kc = rand(3 * STRIDE, n_kv0 * hd, seed=710 + hd, scale=0.3).to(kv_dt)
    vc = rand(3 * STRIDE, n_kv0 * hd, seed=711 + hd).to(kv_dt)
    q = rand(3, H0 * hd, seed=712 + hd)
    want = torch.cat([
        R.attention(q[b: b + 1].cpu(),
                    kc[s * STRIDE: (s + 1) * STRIDE].cpu().float(),
                    vc[s * STRIDE: (s + 1) * STRIDE].cpu().float(),
                    torch.tensor([p]), H0, hd)
        for b, (s, p) in enumerate(zip(ROW_SLOTS, ROW_POS))])
    return q, kc, vc, want


def run_rows(k, shape, q, kc, vc):
    hd, H0, n_kv0 = shape
    z = q80_bufs(3, H0, hd)
    ml, osc, _ = scratch(3, H0, hd)
    k.attn_rows(q, H0 * hd, kc, vc, torch.zeros(3, H0 * hd, device=DEV),
                table([[s * STRIDE, p] for s, p in zip(ROW_SLOTS, ROW_POS)]),
                3, H0, H0 // n_kv0, hd, 1, ml, osc, *z)
    return z


def same(got, want):
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_wide_rows_isolation(k, shape, kv_dt):
    """Every row has its own length and base: the outputs match the
    reference, and no bit changes with what the cache rows outside each
    row's own base..base+pos hold."""
    q, kc, vc, want = rows_case(shape, kv_dt)
    own = torch.zeros(kc.shape[0], dtype=torch.bool, device=DEV)
    for s, p in zip(ROW_SLOTS, ROW_POS):
        own[s * STRIDE: s * STRIDE + p + 1] = True
    z = run_rows(k, shape, q, kc, vc)
    check_q80(z, want, f"rows shape={shape} {kv_dt}")
    for poison in (1e4, -3e4):
        kc_p, vc_p = kc.clone(), vc.clone()
        kc_p[~own] = poison
        vc_p[~own] = poison
        same(run_rows(k, shape, q, kc_p, vc_p), z)


# ------------------------------------------------------------------- paged

def paged_pool(kc, vc, P, share):
    """The three slots' rows scattered into a pool of pages of P rows
    through a seeded permutation of the page ids, with spare pages between.
    share: slot ROW_SLOTS[2]'s first 128 positions are the physical pages of
    slot ROW_SLOTS[1]'s. Returns (pool K, pool V, page table)."""
    pps = STRIDE // P
    g = torch.Generator().manual_seed(720 + P)
    ids = torch.randperm(3 * pps + 5, generator=g)[: 3 * pps].reshape(3, pps)
    if share:
        a, b = ROW_SLOTS[1], ROW_SLOTS[2]
        ids[b, : 128 // P] = ids[a, : 128 // P]
    kp = torch.zeros((3 * pps + 5) * P, kc.shape[1], dtype=kc.dtype, device=DEV)
    vp = torch.zeros_like(kp)
    # pool row of every cache row, slot major (shared pages: equal content)
    dst = (ids.unsqueeze(-1) * P + torch.arange(P)).reshape(-1).to(DEV)
    kp[dst], vp[dst] = kc, vc
    return kp, vp, ids.to(torch.int32).to(DEV).contiguous()


@pytest.mark.parametrize("P,share", [(4, False), (8, False), (64, False),
                                     (8, True)])
@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_wide_paged_equals_rows(k, shape, kv_dt, P, share):
    """Only the addressing differs from the row table, so the bits are the
    same; with share, two rows read their first 128 positions from one set
    of physical pages."""
    hd, H0, n_kv0 = shape
    q, kc, vc, _ = rows_case(shape, kv_dt)
    if share:
        kc, vc = kc.clone(), vc.clone()
        a, b = ROW_SLOTS[1], ROW_SLOTS[2]
        kc[b * STRIDE: b * STRIDE + 128] = kc[a * STRIDE: a * STRIDE + 128]
        vc[b * STRIDE: b * STRIDE + 128] = vc[a * STRIDE: a * STRIDE + 128]
    want = run_rows(k, shape, q, kc, vc)
    kp, vp, pt = paged_pool(kc, vc, P, share)
    z = q80_bufs(3, H0, hd)
    ml, osc, _ = scratch(3, H0, hd)
    rows = table([[s * (STRIDE // P), p] for s, p in zip(ROW_SLOTS, ROW_POS)])
    k.attn_paged(q, H0 * hd, kp, vp, torch.zeros(3, H0 * hd, device=DEV),
                 rows, pt, P, 3, H0, H0 // n_kv0, hd, 1, ml, osc, *z)
    same(z, want)


# ----------------------------------------------------------- graph capture

@pytest.mark.parametrize("kv_dt", KV_DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_wide_graph_replay(k, shape, kv_dt):
    """A launch captured at pos 10 replays correctly at any position: the
    kernel reads the position from the device and its grid does not depend
    on it."""
    hd, H0, n_kv0 = shape
    q, kc, vc = seq_case(shape, kv_dt)
    pos_t = table([10])
    z = q80_bufs(1, H0, hd)
    y = torch.zeros(1, H0 * hd, device=DEV)
    sc = scratch(1, H0, hd)

    def launch():
        k.attn(q, H0 * hd, kc, vc, y, pos_t, 1, H0, H0 // n_kv0, hd, 1, *sc,
               *z)

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
        same(got, run_seq(k, shape, kv_dt, table([pos]), 1))
