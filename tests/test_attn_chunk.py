"""The tiled MFMA chunk attention (attn_chunk, attn_chunk_rows) against
R.attention on the CPU over the f16 cache values cast to float, with q
replaced by f16(q * scale) / scale, the kernel's one operand rounding.

Per output element, with Vmax the largest |v| of that element over the
timesteps the row attends:
  |got - want| <= 1e-4 + 1e-3 * |want| + 2^-10 * Vmax
the f32 attention tolerance (tests/test_attn_wide.py) plus the rounding of P
to f16: each weight carries at most 2^-11 relative error, the output is a
convex combination of v, and the factor 2 covers second-order terms and
weights below the f16 range. No element is exempt."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd.ops import reference as R

DEV = "cuda"
# (head_dim, n_heads0, n_kv_heads0): kv_mul 4, 2, 2, 1
SHAPES = [(128, 8, 2), (128, 4, 2), (64, 2, 1), (64, 2, 2)]
BATCHES = [1, 2, 31, 32]
POSITIONS = [0, 1, 31, 32, 33, 255, 570]
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


def want_and_bound(q, kc, vc, positions, H0, hd):
    """R.attention of CPU rows and the per-element bound."""
    scale = 1.0 / hd ** 0.5
    want = R.attention((q * scale).half().float() / scale, kc.float(),
                       vc.float(), torch.tensor(positions), H0, hd)
    kv_mul = H0 // (kc.shape[1] // hd)
    vmax = vc.float().abs().cummax(dim=0).values[positions]  # [B, kv_dim0]
    vmax = vmax.reshape(len(positions), -1, 1, hd).expand(-1, -1, kv_mul, -1)
    bound = 1e-4 + 1e-3 * want.abs() + 2.0 ** -10 * vmax.reshape(want.shape)
    return want, bound


def check_y(y, want, bound, what):
    err = (y.cpu() - want).abs()
    print(f"{what}: max err {err.max().item():.3e}, least slack "
          f"{(bound - err).min().item():.3e}")
    assert (err <= bound).all(), what


def check_q80(z, want, bound, what):
    """The block bound of tests/test_attn_wide.py with the attention term
    replaced by `bound`; the scale may move by the block's largest bound."""
    zq, zs, zbs = (t.cpu() for t in z)
    B, n = want.shape
    wb, bb = want.reshape(B, n // 32, 32), bound.reshape(B, n // 32, 32)
    codes = zq.reshape(B, n // 32, 32).float()
    d = zs.unsqueeze(-1)
    err = (codes * d - wb).abs()
    d_want = wb.abs().amax(dim=-1) / 127
    print(f"{what}: max err {err.max().item():.3e}, least slack "
          f"{(0.5 * d + bb - err).min().item():.3e}")
    assert (err <= 0.5 * d + bb).all(), what
    assert ((zs - d_want).abs() <= bb.amax(dim=-1) / 127 + 1e-6).all(), what
    assert torch.equal(zbs, codes.sum(dim=-1)), what


def bufs(B, H0, hd, S):
    """y, the split scratch pair and the Q80 triple."""
    nb = H0 * hd // 32
    return (torch.zeros(B, H0 * hd, device=DEV),
            (torch.zeros(B * H0 * S * 2, device=DEV),
             torch.zeros(B * H0 * S * hd, device=DEV)),
            (torch.zeros(B, H0 * hd, dtype=torch.int8, device=DEV),
             torch.zeros(B, nb, device=DEV), torch.zeros(B, nb, device=DEV)))


# ------------------------------------------------------------ one sequence

@functools.lru_cache(maxsize=None)
def seq_case(shape):
    """q of 32 rows and one sequence's caches (test_attn_wide.py's seeds)."""
    hd, H0, n_kv0 = shape
    kc = rand(SEQ, n_kv0 * hd, seed=700 + hd, scale=0.3).half()
    vc = rand(SEQ, n_kv0 * hd, seed=701 + hd).half()
    return rand(32, H0 * hd, seed=702 + hd), kc, vc


@functools.lru_cache(maxsize=None)
def seq_want(shape, pos):
    """32 rows at pos..pos+31; row b is the same in every batch size."""
    hd, H0, _ = shape
    q, kc, vc = seq_case(shape)
    return want_and_bound(q.cpu(), kc.cpu(), vc.cpu(),
                          list(range(pos, pos + 32)), H0, hd)


def run_seq(k, shape, pos_t, B, S, quant=False):
    hd, H0, n_kv0 = shape
    q, kc, vc = seq_case(shape)
    y, sc, z = bufs(B, H0, hd, S)
    k.attn_chunk(q, H0 * hd, kc, vc, y, pos_t, B, H0, H0 // n_kv0, hd, S, *sc,
                 *(z if quant else ()))
    return z if quant else y


@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_chunk_matches_reference(k, shape, B, pos, S):
    """Row b attends to positions 0..pos+b."""
    want, bound = seq_want(shape, pos)
    y = run_seq(k, shape, table([pos]), B, S)
    check_y(y, want[:B], bound[:B], f"shape={shape} B={B} pos={pos} S={S}")


@pytest.mark.parametrize("shape", SHAPES)
def test_attn_chunk_q80_output(k, shape):
    want, bound = seq_want(shape, 255)
    z = run_seq(k, shape, table([255]), 31, 8, quant=True)
    check_q80(z, want[:31], bound[:31], f"q80 shape={shape}")


# --------------------------------------------------------------- row table

STRIDE = 320  # cache rows per slot
# (slot, positions) per run, slots out of order
LAYOUTS = {
    "chunks": [(2, list(range(5))), (0, [300]), (1, list(range(250, 277)))],
    "scattered": [(1, [3, 40, 41, 100, 7, 64]), (0, [310, 0, 33, 32, 31])],
}


@functools.lru_cache(maxsize=None)
def rows_case(shape, layout):
    hd, H0, n_kv0 = shape
    kc = rand(3 * STRIDE, n_kv0 * hd, seed=710 + hd, scale=0.3).half()
    vc = rand(3 * STRIDE, n_kv0 * hd, seed=711 + hd).half()
    runs = LAYOUTS[layout]
    B = sum(len(p) for _, p in runs)
    q = rand(B, H0 * hd, seed=712 + hd)
    wants, b = [], 0
    for s, ps in runs:
        sl = slice(s * STRIDE, (s + 1) * STRIDE)
        wants.append(want_and_bound(q[b: b + len(ps)].cpu(), kc[sl].cpu(),
                                    vc[sl].cpu(), ps, H0, hd))
        b += len(ps)
    return q, kc, vc, [torch.cat(t) for t in zip(*wants)]


def run_rows(k, shape, layout, q, kc, vc, S=8):
    hd, H0, n_kv0 = shape
    runs = LAYOUTS[layout]
    rows = [[s * STRIDE, p] for s, ps in runs for p in ps]
    first = [sum(len(p) for _, p in runs[:i]) for i in range(len(runs))]
    y, sc, _ = bufs(len(rows), H0, hd, S)
    k.attn_chunk_rows(q, H0 * hd, kc, vc, y, table(rows),
                      table([[f, len(ps)] for f, (_, ps) in zip(first, runs)]),
                      len(runs), len(rows), H0, H0 // n_kv0, hd, S, *sc)
    return y


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("shape", SHAPES)
def test_attn_chunk_rows_isolation(k, shape, layout):
    """Matches the reference, and no bit changes with what the cache rows
    outside each row's own base..base+pos hold."""
    q, kc, vc, (want, bound) = rows_case(shape, layout)
    y = run_rows(k, shape, layout, q, kc, vc)
    check_y(y, want, bound, f"rows shape={shape} {layout}")
    own = torch.zeros(kc.shape[0], dtype=torch.bool, device=DEV)
    for s, ps in LAYOUTS[layout]:
        own[s * STRIDE: s * STRIDE + max(ps) + 1] = True
    for poison in (1e4, -3e4):
        kc_p, vc_p = kc.clone(), vc.clone()
        kc_p[~own] = poison
        vc_p[~own] = poison
        assert torch.equal(run_rows(k, shape, layout, q, kc_p, vc_p), y)


# ----------------------------------------------------------- graph capture

@pytest.mark.parametrize("shape", SHAPES[1:3])
def test_attn_chunk_graph_replay(k, shape):
    """Captured at position 32, replayed elsewhere: equal to eager."""
    hd, H0, n_kv0 = shape
    q, kc, vc = seq_case(shape)
    pos_t = table([32])
    y, sc, _ = bufs(32, H0, hd, 8)

    def launch():
        k.attn_chunk(q, H0 * hd, kc, vc, y, pos_t, 32, H0, H0 // n_kv0, hd, 8,
                     *sc)

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
        assert torch.equal(y.clone(), run_seq(k, shape, table([pos]), 32, 8))


# ---------------------------------------------------------------- refusals

def _h(*shape, dt=torch.float16):
    return lambda: torch.zeros(*shape, dtype=dt, device=DEV)


_i32 = torch.int32
REFUSED = {  # what differs from a valid call of either binding
    "f32 cache": dict(kc=_h(64, 64, dt=torch.float32)),
    "int8 cache": dict(kc=_h(64, 64, dt=torch.int8)),
    "scales": dict(scales=_h(64, 2)),
    "head_dim": dict(hd=32, kc=_h(64, 32)),
    "long run": dict(B=33),
    "runs int64": dict(runs=_h(1, 2, dt=torch.int64)),
    "runs 1-d": dict(runs=_h(2, dt=_i32)),
    "runs strided": dict(runs=lambda: _h(1, 4, dt=_i32)()[:, ::2]),
    "runs short": dict(runs=_h(0, 2, dt=_i32)),
    "runs on cpu": dict(runs=lambda: torch.zeros(1, 2, dtype=_i32)),
}


@pytest.mark.parametrize("what,rows_form", [
    (w, r) for w in REFUSED for r in (False, True) if r or "runs" not in w])
def test_attn_chunk_refuses(k, what, rows_form):
    a = dict(kc=_h(64, 64), hd=64, B=4, runs=_h(1, 2, dt=_i32), scales=None)
    a.update(REFUSED[what])
    hd, B, kc = a["hd"], a["B"], a["kc"]()
    y, sc, _ = bufs(B, 2, hd, 1)
    q = torch.zeros(B, 2 * hd, device=DEV)
    kw = dict(k_scales=a["scales"](), v_scales=a["scales"]()) if a["scales"] else {}
    where = ((table([[0, b] for b in range(B)]), a["runs"](), 1) if rows_form
             else (table([0]),))
    fn = k.attn_chunk_rows if rows_form else k.attn_chunk
    with pytest.raises(RuntimeError, match="run table|attn"):
        fn(q, 2 * hd, kc, kc.clone(), y, *where, B, 2, 2, hd, 1, *sc, **kw)
