"""The shared-prefix attention (attn_prefix_paged: k_attn_prefix over the
pages a group of rows has in common, k_attn_gqa over every row's own suffix,
k_attn_combine_pre) against a float64 softmax attention of every row over
its full history, gathered through its page list; for a Q80 cache over
f16(code * scale). The bound is check_y's (tests/test_attn_chunk.py),
unchanged: the rounding points are the chunk kernel's, q * scale and P to
f16, and the prefix / suffix merge is f32 only.

The pool is poisoned: every row no member may read holds 1e4 (Q80: code 127
with an inf scale), and page ids are dealt so that no two consecutive table
entries are neighbours in memory."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_attn_chunk import DEV, bufs, check_q80, check_y, k, rand  # noqa: F401

HEADS = [(64, 1), (128, 4), (64, 8), (128, 16)]  # (head_dim, kv_mul)
PAGES = [(4, 5), (16, 3), (64, 2)]  # (page size, shared pages of group A)
N_KV = 2


def layout(P, n_pre):
    """The step of 7 rows: (group or None, position) per row and the shared
    pages per group. Group A = rows 0, 3, 5, group B = rows 1, 6 with one
    page less; rows 2 and 4 share nothing. Row 3 sits at pos == plen (a
    suffix of one token), row 5's suffix spans three pages."""
    a, b = n_pre * P, (n_pre - 1) * P
    return ([("A", a + P // 2), ("B", b + 3), (None, 37), ("A", a),
             (None, 2 * P + 5), ("A", a + 2 * P + 1), ("B", b + P + 1)],
            {"A": n_pre, "B": n_pre - 1})


def step_tables(rows, shared, P, cut=128):
    """pre_rows, groups, members, n_groups as the host stages them, groups of
    more than `cut` members cut in row order."""
    pre = [[-1, 0] for _ in rows]
    groups, members = [], []
    for g in shared:
        mine = [b for b, (key, _) in enumerate(rows) if key == g]
        for i in range(0, len(mine), cut):
            for b in mine[i: i + cut]:
                pre[b] = [len(groups), shared[g] * P]
            groups.append([len(members), len(mine[i: i + cut])])
            members += mine[i: i + cut]
    n = len(groups)
    groups += [[0, 0]] * (max(len(rows) // 2, n) - n)
    members += [0] * (len(rows) - len(members))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    return [i32(pre), i32(groups), i32(members), i32([n])]


@functools.lru_cache(maxsize=None)
def case(hd, kv_mul, P, q80, rows, shared):
    """(q, planes [K, V (, K scales, V scales)], page table, want, bound)."""
    shared = dict(shared)
    H0, w = N_KV * kv_mul, N_KV * hd
    need = [pos // P + 1 for _, pos in rows]
    n_alloc = sum(shared.values()) + sum(
        n - shared.get(g, 0) for n, (g, _) in zip(need, rows))
    # odd ids in a shuffled order: every even page is nobody's (poison), so
    # no two mapped pages are neighbours
    mod = n_alloc + (n_alloc % 7 == 0)
    ids = iter(1 + 2 * (j * 7 % mod) for j in range(n_alloc))
    own = {g: [next(ids) for _ in range(n)] for g, n in shared.items()}
    lists = [own.get(g, []) + [next(ids) for _ in range(n - shared.get(g, 0))]
             for n, (g, _) in zip(need, rows)]
    pt = torch.zeros(len(rows), max(need), dtype=torch.int32)
    n_rows = 2 * mod * P
    readable = torch.zeros(n_rows, dtype=torch.bool)
    for b, ((_, pos), pages) in enumerate(zip(rows, lists)):
        pt[b, :len(pages)] = torch.tensor(pages, dtype=torch.int32)
        for t in range(pos + 1):
            readable[pages[t // P] * P + t % P] = True
    readable = readable.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(900 + hd + kv_mul + P)
    if q80:
        planes = [torch.randint(-100, 128, (n_rows, w), device=DEV, generator=g)
                  .to(torch.int8) for _ in range(2)]
        planes += [(a / 127 * (0.5 + torch.rand(n_rows, w // 32, device=DEV,
                                                generator=g))).half()
                   for a in (0.3, 1.0)]
        kv = [(c.float() * s.float().repeat_interleave(32, 1)).half().double()
              .cpu() for c, s in zip(planes[:2], planes[2:])]
        for x in planes:
            x[~readable] = 127 if x.dtype == torch.int8 else float("inf")
    else:  # asymmetric: a sign or an offset error cannot cancel
        planes = [(rand(n_rows, w, seed=910 + hd + P, scale=0.3) + 0.1).half(),
                  (rand(n_rows, w, seed=911 + hd + P) + 0.5).half()]
        kv = [x.double().cpu() for x in planes]
        for x in planes:
            x[~readable] = 1e4
    q = rand(len(rows), H0 * hd, seed=912 + hd + kv_mul)
    scale = 1.0 / hd ** 0.5
    qr = ((q * scale).half().double() / scale).cpu().view(len(rows), H0, hd)
    want = torch.zeros(len(rows), H0, hd, dtype=torch.float64)
    vmax = torch.zeros_like(want)
    for b, ((_, pos), pages) in enumerate(zip(rows, lists)):
        src = torch.tensor([pages[t // P] * P + t % P for t in range(pos + 1)])
        kb, vb = (x[src].view(pos + 1, N_KV, hd) for x in kv)
        for h in range(H0):
            p = torch.softmax(kb[:, h // kv_mul] @ qr[b, h] * scale, dim=0)
            want[b, h] = p @ vb[:, h // kv_mul]
            vmax[b, h] = vb[:, h // kv_mul].abs().amax(dim=0)
    want, vmax = (x.view(len(rows), -1).float() for x in (want, vmax))
    return (q, planes, pt.to(DEV), want,
            1e-4 + 1e-3 * want.abs() + 2.0 ** -10 * vmax)


def launch(k, hd, kv_mul, P, c, rows, tables, S, S_pre, quant=False, tab=None):
    q, planes, pt = c[:3]
    B, H0 = len(rows), N_KV * kv_mul
    if tab is None:
        tab = torch.tensor([[b * pt.shape[1], pos]
                            for b, (_, pos) in enumerate(rows)],
                           dtype=torch.int32, device=DEV)
    y, sc, z = bufs(B, H0, hd, S)
    pre = bufs(B, H0, hd, S_pre)[1]
    for x in pre:
        x.fill_(float("nan"))  # nothing unwritten may be read
    scales = dict(k_scales=planes[2], v_scales=planes[3]) if planes[2:] else {}
    k.attn_prefix_paged(q, H0 * hd, *planes[:2], y, tab, pt, P, *tables, B, H0,
                        kv_mul, hd, S, *sc, S_pre, *pre,
                        *(z if quant else ()), **scales)
    return z if quant else y


@pytest.mark.parametrize("q80", [False, True], ids=["f16", "q80"])
@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("S_pre", [1, 8])
@pytest.mark.parametrize("P,n_pre", PAGES)
@pytest.mark.parametrize("hd,kv_mul", HEADS)
def test_attn_prefix_matches_reference(k, hd, kv_mul, P, n_pre, S_pre, S, q80):
    """Two groups, two ungrouped rows, 12 * kv_mul / 4 live columns: a dead
    wave at small kv_mul, a masked tile at plen 20, empty splits at S_pre 8."""
    rows, shared = layout(P, n_pre)
    c = case(hd, kv_mul, P, q80, tuple(rows), tuple(shared.items()))
    tables = step_tables(rows, shared, P)
    what = f"hd={hd} kv_mul={kv_mul} P={P} S_pre={S_pre} S={S} q80={q80}"
    check_y(launch(k, hd, kv_mul, P, c, rows, tables, S, S_pre), *c[3:], what)
    if (S, S_pre) == (8, 8):  # and the Q80 output triple
        z = launch(k, hd, kv_mul, P, c, rows, tables, S, S_pre, quant=True)
        check_q80(z, *c[3:], "triple " + what)


@pytest.mark.parametrize("q80", [False, True], ids=["f16", "q80"])
def test_attn_prefix_cut_group(k, q80):
    """33 rows behind one prefix at kv_mul 4: 32 members fill the 128 columns
    of one workgroup, the 33rd is a group of its own."""
    P, n_pre = 16, 3
    rows = [("A", n_pre * P + b % 16) for b in range(33)]
    c = case(128, 4, P, q80, tuple(rows), (("A", n_pre),))
    tables = step_tables(rows, {"A": n_pre}, P, cut=32)
    assert tables[1][:2].tolist() == [[0, 32], [32, 1]]
    check_y(launch(k, 128, 4, P, c, rows, tables, 2, 2), *c[3:], f"q80={q80}")


def test_attn_prefix_graph_replay(k):
    """Captured with no live group, replayed with the two groups and again
    with other positions and group A alone: equal to eager each time."""
    hd, kv_mul, (P, n_pre) = 128, 4, PAGES[1]
    rows, shared = layout(P, n_pre)
    c = case(hd, kv_mul, P, False, tuple(rows), tuple(shared.items()))
    pt = c[2]
    tab = torch.tensor([[b * pt.shape[1], pos] for b, (_, pos) in enumerate(rows)],
                       dtype=torch.int32, device=DEV)
    live = step_tables(rows, {}, P)
    B, H0 = len(rows), N_KV * kv_mul
    y, sc, _ = bufs(B, H0, hd, 8)
    pre = bufs(B, H0, hd, 8)[1]
    go = lambda: k.attn_prefix_paged(c[0], H0 * hd, *c[1], y, tab, pt, P, *live,
                                     B, H0, kv_mul, hd, 8, *sc, 8, *pre)
    go()
    torch.cuda.synchronize()
    check_y(y, *c[3:], "no group")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        go()
    # the second step: rows 2 and 4 one position back (the same pages, so
    # the same pool: its reference holds for c's planes), group B not staged
    back = [(key, pos - (key is None)) for key, pos in rows]
    c2 = case(hd, kv_mul, P, False, tuple(back), tuple(shared.items()))
    assert torch.equal(c2[2], pt)
    only_a = [(key if key == "A" else None, pos) for key, pos in back]
    for step, sh, ref in ((rows, shared, c), (only_a, {"A": n_pre}, c2)):
        for dst, src in zip(live, step_tables(step, sh, P)):
            dst.copy_(src)
        tab[:, 1] = torch.tensor([pos for _, pos in step], dtype=torch.int32)
        g.replay()
        check_y(y, *ref[3:], f"replay {sorted(sh)}")
        want = launch(k, hd, kv_mul, P, c, step, step_tables(step, sh, P), 8, 8)
        assert torch.equal(y, want), sh


@pytest.mark.parametrize("hd,kv_mul,dt", [
    (64, 2, torch.float32), (32, 2, torch.float16), (64, 32, torch.float16)],
    ids=["f32", "head_dim", "kv_mul"])
def test_attn_prefix_refuses(k, hd, kv_mul, dt):
    H0 = kv_mul
    kc = torch.zeros(64, hd, dtype=dt, device=DEV)
    y, sc, _ = bufs(2, H0, hd, 2)
    q = torch.zeros(2, H0 * hd, device=DEV)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="attn_prefix_paged"):
        k.attn_prefix_paged(q, H0 * hd, kc, kc.clone(), y, i32(2, 2), i32(2, 4),
                            16, i32(2, 2), i32(1, 2), i32(2), i32(1), 2, H0,
                            kv_mul, hd, 2, *sc, 2, *bufs(2, H0, hd, 2)[1])
