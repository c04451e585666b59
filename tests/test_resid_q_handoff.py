"""The hand-off form of q40_gemv_resid_q (4- or 8-wave workgroups, the last
arriver at a block's ticket emits the Q80 block) against the 16-wave form
that assembles the block in one workgroup's LDS, and against the separate
kernels. Both forms fold a row in the same wave with the same summation
order, so x and the Q80 triple are compared bit for bit; ssq differs by the
order of its float atomics (rtol 1e-4, as in test_hip_ops).

The 16-wave outputs come from one child process run with
DLLAMA_RESID_Q_WAVES=16 (the option is read once per process); this process
runs the default rule and, through q40_gemv_resid_q_waves(), 4 and 8 waves.
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (d, n): one block with an odd trailing Q40 block; test_hip_ops' shape;
# two blocks; the 8B down-projections (128 blocks over all XCDs)
SHAPES = [(32, 32), (96, 160), (64, 64), (4096, 4096), (4096, 14336)]
# 0 = the default rule. It picks the 16-wave kernel at every shape here but
# (4096, 14336), so its other cases only hold the rule to the reference; the
# hand-off itself is covered by forms 4 and 8 at every shape.
FORMS = [0, 4, 8]


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g) * scale


def _q80_bufs(rows, n):
    return (torch.zeros(rows, n, dtype=torch.int8, device=DEV),
            torch.zeros(rows, n // 32, device=DEV),
            torch.zeros(rows, n // 32, device=DEV))


def _q80(k, x):
    out = _q80_bufs(*x.shape)
    k.q80_quantize(x.contiguous(), *out)
    return out


def _ssq_buf(rows=1):
    return torch.zeros(rows, 16 * 32, device=DEV)


def _ssq_total(ssq):
    return ssq.cpu().reshape(-1, 16, 32)[:, :, 0].sum(-1)


def _case(k, d, n):
    """Inputs of one shape, the same in every process: random Q40 planes
    (any nibbles and small f16 scales are a valid matrix), a Q80 input
    triple, the residual row and the norm weight."""
    g = torch.Generator(device=DEV).manual_seed(1000 + d + n)
    qs = torch.randint(0, 256, (d, n // 2), dtype=torch.uint8, device=DEV,
                       generator=g)
    sc = (torch.rand((d, n // 32), device=DEV, generator=g) * 0.02
          ).to(torch.float16)
    xin = _q80(k, _rand(1, n, seed=2000 + d + n, scale=0.5))
    x0 = _rand(1, d, seed=3000 + d + n)
    wnorm = _rand(d, seed=4000 + d + n).abs() + 0.5
    return qs, sc, xin, x0, wnorm


def _run(k, case, x=None):
    """One launch on a fresh copy of x0 (or on x): (x, ssq, codes, scales,
    blocksums)."""
    qs, sc, xin, x0, wnorm = case
    x = x0.clone() if x is None else x
    ssq, out = _ssq_buf(), _q80_bufs(1, x0.shape[1])
    k.q40_gemv_resid_q(qs, sc, *xin, x, ssq, wnorm, *out)
    return (x, ssq) + out


def _assert_same(got, want):
    for name, g, w in zip(("x", "ssq", "codes", "scales", "blocksums"),
                          got, want):
        if name == "ssq":
            assert torch.allclose(_ssq_total(g), _ssq_total(w), rtol=1e-4)
        else:
            g, w = g.cpu(), w.cpu()
            assert torch.equal(g, w), \
                (name, (g.float() - w.float()).abs().max().item())


@pytest.fixture(scope="module")
def k():
    from dllama_amd.ops import hip_ops
    return hip_ops()


@pytest.fixture
def form(k, request):
    k.q40_gemv_resid_q_waves(request.param)
    yield request.param
    k.q40_gemv_resid_q_waves(0)


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    """{(d, n): outputs of the 16-wave form}, computed once by a child
    process that runs this file with the option set."""
    path = str(tmp_path_factory.mktemp("resid_q") / "wide.pt")
    env = dict(os.environ, DLLAMA_RESID_Q_WAVES="16")
    subprocess.run([sys.executable, os.path.abspath(__file__), path],
                   check=True, env=env, timeout=300)
    return torch.load(path)


def _dump_all(path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from dllama_amd.ops import hip_ops
    k = hip_ops()
    out = {}
    for d, n in SHAPES:
        out[(d, n)] = tuple(t.cpu() for t in _run(k, _case(k, d, n)))
    torch.save(out, path)


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("d,n", SHAPES)
def test_equals_16_wave_form(k, wide, form, d, n):
    _assert_same(_run(k, _case(k, d, n)), wide[(d, n)])


@pytest.mark.parametrize("d,n", SHAPES[:3])
def test_option_in_process_is_the_16_wave_form(k, wide, d, n):
    """q40_gemv_resid_q_waves(16) selects what the environment option
    selects: the reference of this file is the 16-wave kernel."""
    k.q40_gemv_resid_q_waves(16)
    try:
        _assert_same(_run(k, _case(k, d, n)), wide[(d, n)])
    finally:
        k.q40_gemv_resid_q_waves(0)


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_against_separate_kernels(k, form):
    """q40_gemv_resid, then Q80 of x*wnorm, as test_q40_gemv_resid_q."""
    case = _case(k, 96, 160)
    qs, sc, xin, x0, wnorm = case
    xa, ssq_a = x0.clone(), _ssq_buf()
    k.q40_gemv_resid(qs, sc, *xin, xa, ssq_a, 1)
    xb, ssq_b, *out = _run(k, case)
    assert torch.equal(xb, xa), (xb - xa).abs().max().item()
    want_ssq = (xa.cpu() ** 2).sum(-1)
    assert torch.allclose(_ssq_total(ssq_b), want_ssq, rtol=1e-4)
    for name, g, w in zip(("codes", "scales", "blocksums"), out,
                          _q80(k, xb * wnorm)):
        assert torch.equal(g, w), name


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("d,n", [(96, 160), (4096, 4096)])
def test_tickets_return_to_rest(k, form, d, n):
    """64 back-to-back launches, no reset between them: on fresh copies of
    x0, on one buffer refilled from x0 (the same tickets 64 times), and the
    latter captured in one graph and replayed three times."""
    case = _case(k, d, n)
    qs, sc, xin, x0, wnorm = case
    first = _run(k, case)
    for _ in range(64):
        _assert_same(_run(k, case), first)
    N = 64
    x = x0.clone()
    xs = torch.zeros(N, d, device=DEV)
    ssq = _ssq_buf(N)
    oq, os_, obs = _q80_bufs(N, d)

    def burst():
        for i in range(N):
            x.copy_(x0)
            k.q40_gemv_resid_q(qs, sc, *xin, x, ssq[i], wnorm,
                               oq[i], os_[i], obs[i])
            xs[i].copy_(x[0])

    def check():
        torch.cuda.synchronize()
        want_ssq = _ssq_total(first[1]).expand(N)
        assert torch.allclose(_ssq_total(ssq), want_ssq, rtol=1e-4)
        for name, g, w in zip(("x", "codes", "scales", "blocksums"),
                              (xs, oq, os_, obs),
                              (first[0],) + tuple(first[2:])):
            assert torch.equal(g, w.expand_as(g)), name

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        burst()  # eager warm-up: tickets of x exist before the capture
    torch.cuda.current_stream().wait_stream(s)
    check()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        burst()
    for _ in range(3):
        for t in (xs, ssq, oq, os_, obs):
            t.zero_()
        graph.replay()
        check()


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("d,n", [(96, 160), (4096, 4096)])
def test_lines_read_before_each_launch(k, form, d, n):
    """The last arriver must not take its neighbours' rows from lines a CU
    already holds: besides the kernel's own read of its rows, a plain
    elementwise read of all of x runs immediately before each launch."""
    case = _case(k, d, n)
    x0 = case[3]
    first = _run(k, case)
    sink = torch.zeros_like(x0)
    for _ in range(16):
        x = x0.clone()
        torch.add(x, 1.0, out=sink)
        _assert_same(_run(k, case, x), first)
        assert torch.equal(sink, x0 + 1.0)


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_tickets_belong_to_the_residual_buffer(k, form):
    """Two residual buffers of different d, used alternately, each give
    their single-buffer result; so does one address first used with a small
    d and then with a larger one (its ticket array has to grow)."""
    small, big = _case(k, 64, 64), _case(k, 4096, 4096)
    want_small, want_big = _run(k, small), _run(k, big)
    xs_, xb_ = small[3].clone(), big[3].clone()
    for _ in range(8):
        xs_.copy_(small[3])
        _assert_same(_run(k, small, xs_), want_small)
        xb_.copy_(big[3])
        _assert_same(_run(k, big, xb_), want_big)
    buf = torch.zeros(1, 4096, device=DEV)
    for _ in range(2):
        buf[:, :64].copy_(small[3])
        got = _run(k, small, buf)
        _assert_same((got[0][:, :64],) + got[1:], want_small)
        buf.copy_(big[3])
        _assert_same(_run(k, big, buf), want_big)


def test_first_use_inside_capture_is_refused(k):
    """Tickets are allocated and zeroed outside stream capture; a residual
    buffer whose first launch is inside a capture gets a clear error."""
    k.q40_gemv_resid_q_waves(4)
    try:
        case = _case(k, 64, 64)
        qs, sc, xin, x0, wnorm = case
        # a row inside a large allocation: an address no launch has used
        x = torch.zeros(3, 1 << 19, device=DEV)[1:2]
        ssq, out = _ssq_buf(), _q80_bufs(1, 64)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ssq.zero_()
            with pytest.raises(RuntimeError, match="stream capture"):
                k.q40_gemv_resid_q(qs, sc, *xin, x, ssq, wnorm, *out)
    finally:
        k.q40_gemv_resid_q_waves(0)


if __name__ == "__main__":
    _dump_all(sys.argv[1])
