"""The Q80 form of the GQA-packed MFMA decode attention against R.attention on
f16(code * scale), with the cases and the bound of tests/test_attn_gqa.py."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_attn_chunk import (DEV, bufs, check_q80, check_y, k, rand,  # noqa: F401
                             table, want_and_bound)
from test_attn_gqa import (B, FORMS, MAXPOS, POSITIONS, ROWS, SEQ, SHAPES,
                           STRIDE, form_case)

POISONS = ((127, 1e4), (-127, float("inf")))  # codes, scales


@functools.lru_cache(maxsize=None)
def planes(shape, n):
    """q of len(ROWS) rows and n cache rows: K, V codes, K, V scales."""
    hd, H0, n_kv0 = shape
    w, g = n_kv0 * hd, torch.Generator(device=DEV).manual_seed(820 + hd + n)
    codes = [torch.randint(-127, 128, (n, w), device=DEV, generator=g)
             .to(torch.int8) for _ in range(2)]
    return rand(len(ROWS), H0 * hd, seed=822 + hd + H0), codes + [
        (a / 127 * (0.5 + torch.rand(n, w // 32, device=DEV, generator=g)))
        .half() for a in (0.3, 1.0)]


@functools.lru_cache(maxsize=None)
def want(shape, n, b0, first, positions):
    """Of q rows b0.. at `positions` of the sequence from cache row `first`."""
    q, p = planes(shape, n)
    kv = [(c[first:].float() * s[first:].float().repeat_interleave(32, 1))
          .half().cpu() for c, s in zip(p[:2], p[2:])]
    return want_and_bound(q[b0: b0 + len(positions)].cpu(), *kv,
                          list(positions), shape[1], shape[0])


def run(k, shape, form, q, p, where, S=8, quant=False):
    hd, H0, n_kv0 = shape
    y, sc, z = bufs(len(q), H0, hd, S)
    getattr(k, "attn_gqa" + form)(
        q, H0 * hd, *p[:2], y, *where, len(q), H0, H0 // n_kv0, hd, S, *sc,
        *(z if quant else ()), k_scales=p[2], v_scales=p[3])
    return z if quant else y


@pytest.mark.parametrize("S", [2, 8])
@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_gqa_q80_matches_reference(k, shape, pos, S):
    q, p = planes(shape, SEQ)
    w = want(shape, SEQ, 0, 0, tuple(range(pos, pos + B)))
    y = run(k, shape, "", q[:B], p, (table([pos]),), S)
    check_y(y, *w, f"shape={shape} pos={pos} S={S}")
    if (pos, S) == (127, 8):  # and with the Q80 output triple
        z = run(k, shape, "", q[:B], p, (table([pos]),), S, quant=True)
        check_q80(z, *w, f"q80 in and out shape={shape}")


def rows_form(shape, P):
    """test_attn_gqa.form_case's layout: (binding suffix, planes, arguments)."""
    _, where, slot, t = form_case(shape, P)
    src = slot.clamp(min=0) * STRIDE + t
    return ("_paged" if P else "_rows",
            [x[src] for x in planes(shape, 3 * STRIDE)[1]], where)


def run_rows(k, shape, P, p, rows=range(len(ROWS))):
    form, _, where = rows_form(shape, P)
    tab = table([[ROWS[b][0] * STRIDE // (P or 1), ROWS[b][1]] for b in rows])
    q = planes(shape, 3 * STRIDE)[0][list(rows)].contiguous()
    return run(k, shape, form, q, p, (tab, *where))


@pytest.mark.parametrize("P", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_gqa_q80_rows_isolation(k, shape, P):
    """Within the bound; paged equal to unpaged; blind to codes and scales
    outside every row's own 0..pos; a row alone has its bits of the batch."""
    _, _, slot, t = form_case(shape, P)
    p = rows_form(shape, P)[1]
    y = run_rows(k, shape, P, p)
    wants = [want(shape, 3 * STRIDE, b, s * STRIDE, (pos,))
             for b, (s, pos) in enumerate(ROWS)]
    check_y(y, *(torch.cat(x) for x in zip(*wants)), f"shape={shape} P={P}")
    if P:
        assert torch.equal(y, run_rows(k, shape, None,
                                       rows_form(shape, None)[1]))

    def poisoned(own, code, scale):
        bad = [x.clone() for x in p]
        for x in bad:
            x[~own] = code if x.dtype == torch.int8 else scale
        return bad

    readable = t <= torch.tensor(MAXPOS + [-1], device=DEV)[slot]
    for poison in POISONS:
        assert torch.equal(run_rows(k, shape, P, poisoned(readable, *poison)), y)
    for b, (s, pos) in enumerate(ROWS):
        own = (slot == s) & (t <= pos)
        alone = run_rows(k, shape, P, poisoned(own, *POISONS[b % 2]), [b])
        assert torch.equal(alone[0], y[b]), (b, s, pos)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]])
def test_attn_gqa_q80_paged_graph_replay(k, shape):
    """Captured at position 32 with pages of 32 rows, replayed elsewhere."""
    _, p, where = rows_form(shape, 32)
    tab = table([[s * STRIDE // 32, 32] for s, _ in ROWS])
    q = planes(shape, 3 * STRIDE)[0]
    hd, H0, n_kv0 = shape
    y, sc, _ = bufs(len(ROWS), H0, hd, 8)

    def go(y, tab):
        k.attn_gqa_paged(q, H0 * hd, *p[:2], y, tab, *where, len(ROWS), H0,
                         H0 // n_kv0, hd, 8, *sc, k_scales=p[2], v_scales=p[3])
        return y

    go(y, tab)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        go(y, tab)
    for pos in (0, 100):
        tab[:, 1] = pos
        g.replay()
        assert torch.equal(y, go(torch.zeros_like(y), tab.clone())), pos
