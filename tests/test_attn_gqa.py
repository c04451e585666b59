"""The GQA-packed MFMA decode attention (attn_gqa, attn_gqa_rows,
attn_gqa_paged) against R.attention on the CPU, with the oracle and the
per-element bound of tests/test_attn_chunk.py: the kernel has the same
rounding points (q * scale and P to f16) and merges in f32 only."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_attn_chunk import (DEV, bufs, check_q80, check_y, k, rand,  # noqa: F401
                             table, want_and_bound)

# (head_dim, n_heads0, n_kv_heads0): kv_mul 4, 8, 2, 4, 1
SHAPES = [(128, 8, 2), (128, 8, 1), (128, 4, 2), (64, 4, 1), (64, 2, 2)]
POSITIONS = [0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 570]
SEQ, B = 608, 3


@functools.lru_cache(maxsize=None)
def seq_case(shape):
    hd, H0, n_kv0 = shape
    return (rand(B, H0 * hd, seed=802 + hd + H0),
            rand(SEQ, n_kv0 * hd, seed=800 + hd, scale=0.3).half(),
            rand(SEQ, n_kv0 * hd, seed=801 + hd).half())


@functools.lru_cache(maxsize=None)
def seq_want(shape, pos):
    q, kc, vc = seq_case(shape)
    return want_and_bound(q.cpu(), kc.cpu(), vc.cpu(),
                          list(range(pos, pos + B)), shape[1], shape[0])


def run_seq(k, shape, pos_t, S, quant=False):
    hd, H0, n_kv0 = shape
    q, kc, vc = seq_case(shape)
    y, sc, z = bufs(B, H0, hd, S)
    k.attn_gqa(q, H0 * hd, kc, vc, y, pos_t, B, H0, H0 // n_kv0, hd, S, *sc,
               *(z if quant else ()))
    return z if quant else y


@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_gqa_matches_reference(k, shape, pos, S):
    """Row b attends to positions 0..pos+b."""
    y = run_seq(k, shape, table([pos]), S)
    check_y(y, *seq_want(shape, pos), f"shape={shape} pos={pos} S={S}")


@pytest.mark.parametrize("shape", SHAPES)
def test_attn_gqa_q80_output(k, shape):
    z = run_seq(k, shape, table([127]), 8, quant=True)
    check_q80(z, *seq_want(shape, 127), f"q80 shape={shape}")


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]])
def test_attn_gqa_graph_replay(k, shape):
    """Captured at position 32, replayed elsewhere: equal to eager."""
    pos_t = table([32])
    hd, H0, n_kv0 = shape
    q, kc, vc = seq_case(shape)
    y, sc, _ = bufs(B, H0, hd, 8)
    launch = lambda: k.attn_gqa(q, H0 * hd, kc, vc, y, pos_t, B, H0,
                                H0 // n_kv0, hd, 8, *sc)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for pos in (0, 200, 570):
        pos_t.fill_(pos)
        g.replay()
        assert torch.equal(y.clone(), run_seq(k, shape, table([pos]), 8)), pos


STRIDE = 320  # cache rows per slot in the unpaged layout
# (slot, position) per row: slots out of order, 0 and 1 serve two rows each
ROWS = [(2, 100), (0, 276), (1, 33), (0, 31), (1, 300)]
MAXPOS = [276, 300, 100]  # per slot
FORMS = [None, 4, 64]     # unpaged, or rows per page


@functools.lru_cache(maxsize=None)
def rows_case(shape):
    """q, the unpaged caches and (reference, bound) of ROWS."""
    hd, H0, n_kv0 = shape
    kc = rand(3 * STRIDE, n_kv0 * hd, seed=810 + hd, scale=0.3).half()
    vc = rand(3 * STRIDE, n_kv0 * hd, seed=811 + hd).half()
    q = rand(len(ROWS), H0 * hd, seed=812 + hd + H0)
    wants = [want_and_bound(q[b: b + 1].cpu(),
                            kc[s * STRIDE: (s + 1) * STRIDE].cpu(),
                            vc[s * STRIDE: (s + 1) * STRIDE].cpu(), [p], H0, hd)
             for b, (s, p) in enumerate(ROWS)]
    return q, kc, vc, [torch.cat(t) for t in zip(*wants)]


@functools.lru_cache(maxsize=None)
def form_case(shape, P):
    """(caches, arguments behind the row table, slot and timestep of every
    cache row) of one form. Paged: the slots' pages scrambled over a pool;
    page 0 is nobody's (slot -1) and unmapped table entries name it."""
    _, kc, vc, _ = rows_case(shape)
    if P is None:
        r = torch.arange(3 * STRIDE, device=DEV)
        return (kc, vc), (), r // STRIDE, r % STRIDE
    need = [m // P + 1 for m in MAXPOS]
    ids = (torch.randperm(sum(need), generator=torch.Generator()
                          .manual_seed(P)) + 1).tolist()
    pt = torch.zeros(3, STRIDE // P, dtype=torch.int32)
    src = torch.zeros((sum(need) + 1) * P, dtype=torch.long)
    slot = torch.full_like(src, -1)
    for s in range(3):
        for j in range(need[s]):
            pid = ids.pop()
            pt[s, j] = pid
            src[pid * P: (pid + 1) * P] = s * STRIDE + j * P + torch.arange(P)
            slot[pid * P: (pid + 1) * P] = s
    src = src.to(DEV)
    return ((kc[src], vc[src]), (pt.to(DEV), P), slot.to(DEV), src % STRIDE)


def run_rows(k, shape, P, caches, rows=None, S=8):
    """The rows of ROWS named by `rows` (all of them) as one step."""
    hd, H0, n_kv0 = shape
    rows = list(range(len(ROWS))) if rows is None else rows
    q = rows_case(shape)[0][rows].contiguous()
    tab = table([[ROWS[b][0] * STRIDE // (P or 1), ROWS[b][1]] for b in rows])
    y, sc, _ = bufs(len(rows), H0, hd, S)
    getattr(k, "attn_gqa_paged" if P else "attn_gqa_rows")(
        q, H0 * hd, *caches, y, tab, *form_case(shape, P)[1], len(rows), H0,
        H0 // n_kv0, hd, S, *sc)
    return y


@pytest.mark.parametrize("P", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_gqa_rows_isolation(k, shape, P):
    """Within the bound; no bit changes with what the cache rows outside
    every row's own 0..pos hold; a row alone, with everything outside its
    own 0..pos poisoned, has the bits it has in the batch."""
    caches, _, slot, t = form_case(shape, P)
    y = run_rows(k, shape, P, caches)
    check_y(y, *rows_case(shape)[3], f"shape={shape} P={P}")

    def poisoned(own, poison):
        bad = [c.clone() for c in caches]
        for c in bad:
            c[~own] = poison
        return bad

    readable = t <= torch.tensor(MAXPOS + [-1], device=DEV)[slot]
    for poison in (1e4, -3e4):
        assert torch.equal(run_rows(k, shape, P, poisoned(readable, poison)), y)
    for b, (s, p) in enumerate(ROWS):
        own = (slot == s) & (t <= p)
        alone = run_rows(k, shape, P, poisoned(own, (1e4, -3e4)[b % 2]), [b])
        assert torch.equal(alone[0], y[b]), (b, s, p)


@pytest.mark.parametrize("hd,kv_mul,dt", [
    (64, 2, torch.float32), (64, 2, torch.int8), (32, 2, torch.float16),
    (64, 32, torch.float16)], ids=["f32", "int8", "head_dim", "kv_mul"])
def test_attn_gqa_refuses(k, hd, kv_mul, dt):
    H0 = kv_mul
    kc = torch.zeros(64, hd, dtype=dt, device=DEV)
    y, sc, _ = bufs(2, H0, hd, 2)
    q = torch.zeros(2, H0 * hd, device=DEV)
    with pytest.raises(RuntimeError, match="attn_gqa"):
        k.attn_gqa(q, H0 * hd, kc, kc.clone(), y, table([0]), 2, H0, kv_mul,
                   hd, 2, *sc)
