"""attn_chunk_wide (one sequence cut into runs of 32 rows by the kernel)
against R.attention on the CPU, with the q rounding, the comparison and the
per-element bound of tests/test_attn_chunk.py. A Q80 cache enters the
reference as f16(code * scale), the operand the MFMA sees."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_attn_chunk import (DEV, bufs, check_q80, check_y, k, rand,  # noqa: F401
                             table, want_and_bound)

# (head_dim, n_heads0, n_kv_heads0): kv_mul 4 and 1 at both head sizes
SHAPES = [(128, 8, 2), (128, 2, 2), (64, 8, 2), (64, 2, 2)]
# (rows, first position): a second run of one row, two full runs that start
# mid-tile, four runs with a partial last one ending on the cache's last row
CHUNKS = [(33, 0), (64, 5), (97, 31)]
SEQ = 128
S = 4


@functools.lru_cache(maxsize=None)
def case(shape, q80):
    """q of 97 rows, the planes the kernel reads and K, V as the MFMA sees
    them. Built once per key; nothing writes to it."""
    hd, H0, n_kv0 = shape
    w = n_kv0 * hd
    planes = [rand(SEQ, w, seed=730 + hd, scale=0.3).half(),
              rand(SEQ, w, seed=731 + hd).half()]
    seen = planes
    if q80:
        g = torch.Generator(device=DEV).manual_seed(730 + hd)
        planes = [torch.randint(-127, 128, (SEQ, w), device=DEV, generator=g)
                  .to(torch.int8) for _ in range(2)]
        planes += [(a / 127 * (0.5 + torch.rand(SEQ, w // 32, device=DEV,
                                                generator=g))).half()
                   for a in (0.3, 1.0)]
        seen = [(c.float() * s.float().repeat_interleave(32, dim=1)).half()
                for c, s in zip(planes[:2], planes[2:])]
    return rand(97, H0 * hd, seed=732 + hd), planes, [p.cpu() for p in seen]


def run(k, shape, q80, rows, pos, quant=False):  # noqa: F811
    hd, H0, n_kv0 = shape
    q, planes, _ = case(shape, q80)
    y, sc, z = bufs(rows + 1, H0, hd, S)
    y[rows] = 7.0
    k.attn_chunk_wide(q, H0 * hd, *planes[:2], y[:rows], table([pos]), rows, H0,
                      H0 // n_kv0, hd, S, *sc, *(z if quant else ()),
                      **dict(zip(("k_scales", "v_scales"), planes[2:])))
    assert (y[rows] == 7.0).all(), "write past the last row"
    return tuple(t[:rows] for t in z) if quant else y[:rows]


@pytest.mark.parametrize("q80", [False, True])
@pytest.mark.parametrize("rows,pos", CHUNKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_chunk_wide_matches_reference(k, shape, rows, pos, q80):  # noqa: F811
    """Row b attends to positions 0..pos+b, whichever run it falls into."""
    hd, H0, _ = shape
    q, _, (kc, vc) = case(shape, q80)
    want, bound = want_and_bound(q[:rows].cpu(), kc, vc,
                                 list(range(pos, pos + rows)), H0, hd)
    what = f"shape={shape} rows={rows} pos={pos} q80={q80}"
    check_y(run(k, shape, q80, rows, pos), want, bound, what)
    if (rows, pos) == (97, 31):  # and with the Q80 output triple
        check_q80(run(k, shape, q80, rows, pos, quant=True), want, bound, what)
