"""The paged and Q80 forms of the chunk attention against R.attention on the
CPU, with the q rounding and the per-element bound of tests/test_attn_chunk.py.
A Q80 cache enters the reference as f16(code * scale), the operand the MFMA
sees (Vmax over those values). Every form is also bit-blind to the cache rows
no row may read, and the paged form bit-equal to the unpaged one."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_attn_chunk import (DEV, bufs, check_q80, check_y, k, rand,  # noqa: F401
                             table, want_and_bound)

SHAPES = [(128, 8, 2), (64, 2, 1)]
STRIDE = 320  # cache rows per slot in the unpaged layout
# (slot, positions) per run, in table order
RUNS = ((0, tuple(range(250, 277))), (1, (300,)), (2, (3, 40, 41, 100, 7, 64)),
        (1, (0, 31, 32, 33)))
MAXPOS = [276, 300, 100]  # per slot
SHARED = 64  # slot 2's first rows are slot 0's: shared pages when paged
N = sum(len(ps) for _, ps in RUNS)
RUN_TABLE = [[sum(len(p) for _, p in RUNS[:i]), len(ps)]
             for i, (_, ps) in enumerate(RUNS)]


@functools.lru_cache(maxsize=None)
def data(shape, q80):
    """q and the unpaged planes the kernel reads: K, V[, K scales, V scales]."""
    hd, H0, n_kv0 = shape
    n, w = 3 * STRIDE, n_kv0 * hd
    planes = [rand(n, w, seed=720 + hd, scale=0.3).half(),
              rand(n, w, seed=721 + hd).half()]
    if q80:
        g = torch.Generator(device=DEV).manual_seed(720 + hd)
        planes = [torch.randint(-127, 128, (n, w), device=DEV, generator=g)
                  .to(torch.int8) for _ in range(2)]
        planes += [(a / 127 * (0.5 + torch.rand(n, w // 32, device=DEV,
                                                generator=g))).half()
                   for a in (0.3, 1.0)]
    for p in planes:
        p[2 * STRIDE: 2 * STRIDE + SHARED] = p[:SHARED]
    return rand(N, H0 * hd, seed=722 + hd), planes


@functools.lru_cache(maxsize=None)
def paged(shape, q80, P):
    """The slots scattered into a pool of scrambled pages with three unmapped
    ones: (pool planes, page table, mask of the pool rows a row may read)."""
    need, sh = [m // P + 1 for m in MAXPOS], SHARED // P
    ids = torch.randperm(sum(need) - sh + 3,
                         generator=torch.Generator().manual_seed(P)).tolist()
    lists = [ids[:need[0]], ids[need[0]: need[0] + need[1]]]
    lists.append(lists[0][:sh] + ids[need[0] + need[1]:][:need[2] - sh])
    pt = torch.zeros(3, STRIDE // P, dtype=torch.int32)
    src = torch.zeros(len(ids) * P, dtype=torch.long)
    own = torch.zeros(len(ids) * P, dtype=torch.bool)
    for s, pages in enumerate(lists):
        pt[s, :len(pages)] = torch.tensor(pages)
        for j, pid in enumerate(pages):
            t = torch.arange(j * P, (j + 1) * P)
            src[pid * P: (pid + 1) * P] = s * STRIDE + t
            own[pid * P: (pid + 1) * P] = t <= MAXPOS[s]
    return ([p[src.to(DEV)] for p in data(shape, q80)[1]], pt.to(DEV),
            own.to(DEV))


@functools.lru_cache(maxsize=None)
def want(shape, q80, runs=RUNS, stride=STRIDE, P=None):
    """Reference and bound of the rows of `runs`; P: over each slot's rows
    gathered from the pool through its page list."""
    q, planes = data(shape, q80)
    if P:
        pool, pt, _ = paged(shape, q80, P)
        planes = [torch.zeros_like(p) for p in planes]
        for s, m in enumerate(MAXPOS):
            t = torch.arange(m + 1, device=DEV)
            for dst, p in zip(planes, pool):
                dst[s * STRIDE + t] = p[pt[s, t // P].long() * P + t % P]
    if q80:  # K and V as the MFMA sees them
        planes = [(c.float() * s.float().repeat_interleave(32, dim=1)).half()
                  for c, s in zip(planes[:2], planes[2:])]
    out, b = [], 0
    for s, ps in runs:
        kv = [p[s * stride: (s + 1) * stride].cpu() for p in planes]
        out.append(want_and_bound(q[b: b + len(ps)].cpu(), *kv, list(ps),
                                  shape[1], shape[0]))
        b += len(ps)
    return [torch.cat(t) for t in zip(*out)]


def launch(k, shape, form, planes, where, n=N, S=8, quant=False):
    hd, H0, n_kv0 = shape
    y, sc, z = bufs(n, H0, hd, S)
    getattr(k, "attn_chunk" + form)(
        data(shape, len(planes) == 4)[0], H0 * hd, *planes[:2], y, *where, n,
        H0, H0 // n_kv0, hd, S, *sc, *(z if quant else ()),
        **dict(zip(("k_scales", "v_scales"), planes[2:])))
    return z if quant else y


def check_blind(run, planes, own, y):
    """No bit of y changes with what the unreadable rows hold."""
    for poison in (1e4, -3e4):
        bad = [p.clone() for p in planes]
        for p in bad:
            p[~own] = poison if p.dtype == torch.float16 else (
                127 if poison > 0 else -127)
        assert torch.equal(run(bad), y), poison


def rows_form(shape, q80, P=None):
    """(binding suffix, planes, its arguments from rows to n_runs, readable
    rows) of the RUNS step, paged with pages of P rows or unpaged."""
    rows = table([[s * STRIDE // (P or 1), p] for s, ps in RUNS for p in ps])
    if P:
        pool, pt, own = paged(shape, q80, P)
        return "_paged", pool, (rows, pt, P, table(RUN_TABLE), len(RUNS)), own
    own = torch.cat([torch.arange(STRIDE) <= m for m in MAXPOS]).to(DEV)
    return "_rows", data(shape, q80)[1], (rows, table(RUN_TABLE), len(RUNS)), own


# f16 paged: a tile spans 8 pages, is a page, lies inside one; Q80 by table
@pytest.mark.parametrize("q80,P", [(False, 4), (False, 32), (False, 64),
                                   (True, None), (True, 32)])
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_chunk_forms_rows(k, shape, q80, P):
    form, planes, where, own = rows_form(shape, q80, P)
    y = launch(k, shape, form, planes, where)
    check_y(y, *want(shape, q80, P=P), f"shape={shape} q80={q80} P={P}")
    check_blind(lambda p: launch(k, shape, form, p, where), planes, own, y)
    _, flat, flat_where, _ = rows_form(shape, q80)
    assert torch.equal(y, launch(k, shape, "_rows", flat, flat_where))


@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("pos", [0, 31, 32, 33, 255, 570])
@pytest.mark.parametrize("n", [1, 31, 32])
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_chunk_q80_seq(k, shape, n, pos, S):
    """The three slots' rows read as one sequence; row b is position pos+b."""
    planes = data(shape, True)[1]
    run = lambda p: launch(k, shape, "", p, (table([pos]),), n, S)
    w, bound = want(shape, True, ((0, tuple(range(pos, pos + 32))),), 3 * STRIDE)
    y = run(planes)
    check_y(y, w[:n], bound[:n], f"q80 shape={shape} n={n} pos={pos} S={S}")
    check_blind(run, planes, torch.arange(3 * STRIDE, device=DEV) < pos + n, y)
    if (n, pos, S) == (31, 255, 8):  # and with the Q80 output triple
        z = launch(k, shape, "", planes, (table([pos]),), n, S, quant=True)
        check_q80(z, w[:n], bound[:n], f"q80 in and out shape={shape}")


@pytest.mark.parametrize("shape", SHAPES)
def test_attn_chunk_q80_paged_graph_replay(k, shape):
    """Captured once, replayed with other positions and another page table."""
    hd, H0, n_kv0 = shape
    pool, pt, _ = paged(shape, True, 32)
    pt, rows = pt.clone(), table([[0, 32 + i] for i in range(32)])
    q, runs = data(shape, True)[0], table([[0, 32]])
    y, sc, _ = bufs(32, H0, hd, 8)

    def go(y, rows, pt):
        k.attn_chunk_paged(q, H0 * hd, *pool[:2], y, rows, pt, 32, runs, 1,
                           32, H0, H0 // n_kv0, hd, 8, *sc, k_scales=pool[2],
                           v_scales=pool[3])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        go(y, rows, pt)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        go(y, rows, pt)
    for p0 in (0, 200, 100):
        rows[:, 1] = torch.arange(p0, p0 + 32, device=DEV)
        pt[:2] = pt[:2].flip(0)  # table row 0 is now the other slot's pages
        g.replay()
        eager = torch.zeros_like(y)
        go(eager, rows.clone(), pt.clone())
        assert torch.equal(y, eager), p0
