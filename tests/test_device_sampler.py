"""The on-device temperature/top-p sampler (csrc/sampler.hip) against the
float64 oracle `sample_ref` and the host `Sampler`, alone and inside the
captured decode graph.

Coins are placed at the midpoints of the oracle's decision intervals, after
asserting in float64 that every interval is far wider than f32 summation
error, so the kernel is judged only on inputs proven insensitive to it."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dllama_amd import model_file as mf
from dllama_amd.engine import InferenceEngine
from dllama_amd.models.config import ModelConfig
from dllama_amd.ops.reference import sample_ref
from dllama_amd.tokenizer import Sampler
from dllama_amd.utils.testing import make_tiny_llama

T, TOPP = 0.8, 0.9
MAX_COIN = (2 ** 24 - 1) / 2 ** 24  # the largest coin the xorshift draw gives

_samplers = {}


def _dev(v):
    """One DeviceSampler per vocabulary size, shared by every test: its
    scratch (the candidate counter above all) is reused across calls."""
    from dllama_amd.ops.sampler import DeviceSampler
    if v not in _samplers:
        _samplers[v] = DeviceSampler(v, "cuda")
    return _samplers[v]


def _nucleus(logits, temperature=T, topp=TOPP):
    """float64 (order, c, last) of the nucleus rule."""
    x = np.asarray(logits, dtype=np.float64) / temperature
    p = np.exp(x - x.max())
    p /= p.sum()
    idx = np.nonzero(p >= (1.0 - topp) / (len(p) - 1))[0]
    order = idx[np.argsort(-p[idx], kind="stable")]
    c = np.cumsum(p[order])
    last = min(int(np.searchsorted(c, topp, side="right")), len(order) - 1)
    return order, c, last


def _midpoint(c, last, j):
    lo = c[j - 1] if j else 0.0
    return 0.5 * (lo + c[j]) / c[last]


def _randn(v, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(v, generator=g) * scale


# seeds: of 1..9 the one with the longest nucleus that passes the float64
# precondition below (6, 52 and 96 members)
@pytest.mark.parametrize("v,seed", [(33, 3), (1000, 9), (4096, 1)])
def test_midpoint_sweep(v, seed):
    logits = _randn(v, 3.0, seed)
    order, c, last = _nucleus(logits.numpy())
    widths = np.diff(np.concatenate([[0.0], c[: last + 1]])) / c[last]
    assert (0.5 * widths).min() >= 1e-4
    assert np.abs(c - TOPP).min() >= 1e-4
    row, smp = logits.cuda(), _dev(v)
    for j in range(last + 1):
        coin = _midpoint(c, last, j)
        assert sample_ref(logits, T, TOPP, coin)[0] == order[j]
        assert smp.sample(row, coin, T, TOPP) == order[j], j
    assert smp.sample(row, 0.0, T, TOPP) == order[0]
    assert smp.sample(row, MAX_COIN, T, TOPP) == order[last]


def test_ties():
    v = 512
    hot = [3, 64, 65, 130, 255, 256, 400, 511]
    logits = torch.full((v,), -10.0)
    logits[hot] = 2.5
    order, c, last = _nucleus(logits.numpy())
    assert list(order) == hot and last == 7
    row, smp = logits.cuda(), _dev(v)
    for j in range(8):
        assert smp.sample(row, _midpoint(c, last, j), T, TOPP) == hot[j]
    assert smp.sample(row, 0.3, 0.0, TOPP) == hot[0]


def test_uniform():
    v = 64
    row, smp = torch.full((v,), 0.75).cuda(), _dev(v)
    order, c, last = _nucleus(np.full(v, 0.75))
    assert list(order) == list(range(v)) and last == 57
    for j in range(58):
        assert smp.sample(row, _midpoint(c, last, j), T, TOPP) == j
    assert smp.sample(row, MAX_COIN, T, TOPP) == 57


@pytest.mark.parametrize("topp", [1.0, 0.0])
def test_multinomial(topp):
    v = 1000
    logits = _randn(v, 3.0, 77)
    x = logits.numpy().astype(np.float64) / T
    p = np.exp(x - x.max())
    p /= p.sum()
    cdf = np.cumsum(p)
    row, smp = logits.cuda(), _dev(v)
    picked = np.nonzero(p >= 1e-4)[0]
    assert len(picked) > 50
    for i in picked:
        coin = cdf[i] - 0.5 * p[i]
        assert sample_ref(logits, T, topp, coin)[0] == i
        assert smp.sample(row, coin, T, topp) == i
    # no running sum exceeds the coin: the last index
    assert smp.sample(row, 1.5, T, topp) == v - 1


def test_multinomial_more_blocks_than_threads():
    """Past 1024 * 1024 logits the final workgroup scans the per-block sums
    in more than one pass."""
    v = 1024 * 1024 + 1500
    hot = v - 3
    logits = torch.zeros(v)
    logits[hot] = 10.0
    row, smp = logits.cuda(), _dev(v)
    # p[hot] = e^12.5 / (e^12.5 + v - 1) = 0.2035: the cdf jumps over 0.9 there
    tok, margin = sample_ref(logits, T, 1.0, 0.9)
    assert tok == hot and margin > 0.09
    assert smp.sample(row, 0.9, T, 1.0) == hot
    assert smp.sample(row, 0.9, 0.0, 1.0) == hot
    assert smp.sample(row, 0.9, T, TOPP) is None  # every token is a candidate


@pytest.mark.parametrize("v,scale", [(1000, 3.0), (4096, 6.0)])
def test_stream_matches_host_sampler(v, scale):
    n, seed = 100, 12345
    rows = (np.random.default_rng(v).standard_normal((n, v)) * scale).astype(np.float32)
    dev_rows = torch.from_numpy(rows).cuda()
    host = Sampler(v, T, TOPP, seed)
    coins = Sampler(v, T, TOPP, seed)
    smp = _dev(v)
    left_out = 0
    for i in range(n):
        coin = coins.next_coin()
        want = host.sample(rows[i])
        got = smp.sample(dev_rows[i], coin, T, TOPP)
        if sample_ref(rows[i], T, TOPP, coin)[1] < 1e-5:
            left_out += 1
            continue
        assert got == want, i
    assert host.state == coins.state
    assert left_out <= n // 10


def test_cap_boundary():
    from dllama_amd.ops import hip_ops
    v, cap = 16384, int(hip_ops().sampler_max_candidates())
    assert cap == 8192
    perm = torch.randperm(v, generator=torch.Generator().manual_seed(5))
    hot = torch.sort(perm[:cap]).values
    logits = torch.full((v,), -30.0)
    logits[hot] = 0.0
    smp = _dev(v)
    _, c, last = _nucleus(logits.numpy())
    for j in (0, 1, 100):
        assert smp.sample(logits.cuda(), _midpoint(c, last, j), T, TOPP) == int(hot[j])
    assert int(smp.out[1]) == 0
    logits[int(perm[cap])] = 0.0  # one candidate more than the cap holds
    assert smp.sample(logits.cuda(), 0.5, T, TOPP) is None
    assert int(smp.out[1]) == 1
    # and the next call in range starts from a clean counter
    logits[int(perm[cap])] = -30.0
    assert smp.sample(logits.cuda(), _midpoint(c, last, 1), T, TOPP) == int(hot[1])


class _RowModel:
    """The least model the engine's device-sampling path needs: a fixed
    logits row and a DeviceSampler."""

    def __init__(self, row):
        self.row, self.smp = row, _dev(row.numel())
        self.device = row.device
        self.skip_logits = False

    def forward(self, tokens, positions):
        return self.row.repeat(tokens.shape[0], 1)

    def sample_row(self, row, coin, temperature, topp):
        self.result = self.smp.sample(row, coin, temperature, topp)
        return self.result

    def forward_sample(self, *a):
        raise AssertionError("one token only")


def test_overflow_falls_back_to_torch_path():
    v, seed = 151936, 99
    row = _randn(v, 1.0, 3).cuda()
    assert _dev(v).sample(row, 0.5, T, TOPP) is None
    model = _RowModel(row)
    out, _ = InferenceEngine(model, sampler=Sampler(v, T, TOPP, seed)).generate([1], 1)
    assert model.result is None
    assert out == [Sampler(v, T, TOPP, seed).sample_torch(row)]
    # the same row is in range for the other two modes
    assert _dev(v).sample(row, 0.5, 0.0, TOPP) == int(row.argmax())
    x = row.cpu().numpy().astype(np.float64) / T
    p = np.exp(x - x.max())
    p /= p.sum()
    i = int(p.argmax())
    coin = np.cumsum(p)[i] - 0.5 * p[i]
    tok, margin = sample_ref(row.cpu(), T, 1.0, coin)
    assert tok == i and margin >= 1e-4
    assert _dev(v).sample(row, coin, T, 1.0) == i


def test_deterministic():
    v = 4096
    row, smp = _randn(v, 1.0, 8).cuda(), _dev(v)
    order, c, last = _nucleus(row.cpu().numpy())
    assert len(order) > 2048  # a sort of 4096 keys appended in arbitrary order
    got = {smp.sample(row, 0.5, T, TOPP) for _ in range(20)}
    assert len(got) == 1 and None not in got


# ------------------------------------------------------------ in the model

@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("s") / "tiny.m")
    make_tiny_llama(p, vocab_size=256)
    m = mf.ModelFile(p)
    return m, ModelConfig.from_header(m.header)


def _rel_err(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-9)


def _model(tiny, device_sampling, **kw):
    from dllama_amd.models.hip_model import HipTransformer
    model = HipTransformer.from_file(*tiny, **kw)
    model.device_sampling = device_sampling
    return model


def test_graph_replay_follows_parameters(tiny):
    model = _model(tiny, True)
    model.forward(torch.tensor([3, 17, 101]), torch.arange(3))
    model.capture_decode_graph()
    graph = model._graph
    assert model._graph_samples
    eager_launches = []
    smp = model._sampler()
    launch = smp.launch
    smp.launch = lambda row: (eager_launches.append(1), launch(row))[1]
    steps = [(0.8, 0.9), (0.0, 0.9), (1.5, 0.9), (1.5, 1.0), (0.8, 0.9)]
    coins = Sampler(256, 0.8, 0.9, 4321)
    token = 7
    for i, (temp, topp) in enumerate(steps):
        coin = coins.next_coin()
        got = model.forward_sample(torch.tensor([token]), torch.tensor([3 + i]),
                                   coin, temp, topp)
        assert not eager_launches  # the sampler ran inside the replay
        row = model.last_logits().clone()
        want = model.sample_row(row, coin, temp, topp)
        assert eager_launches.pop() == 1
        assert got == want and got is not None, (i, got, want)
        if temp == 0.0:
            assert got == int(row.argmax())
        token = got
    assert model._graph is graph  # no recapture


class _Recording(Sampler):
    """Host sampler that keeps (logits, coin) of every sampled token."""

    def sample_with_coin(self, logits, coin):
        self.seen.append((logits.detach().float().cpu().numpy().copy(), coin))
        return super().sample_with_coin(logits, coin)


def _baseline(model, n, prompt):
    """Host-sampled tokens of the first seed in 1..20 whose every step is
    decided with margin >= 1e-4 in float64; the baseline alone picks it."""
    for seed in range(1, 21):
        sampler = _Recording(256, T, TOPP, seed)
        sampler.seen = []
        out, _ = InferenceEngine(model, sampler=sampler).generate(prompt, n)
        assert len(sampler.seen) == n
        if all(sample_ref(l, T, TOPP, coin)[1] >= 1e-4 for l, coin in sampler.seen):
            return seed, out
    raise AssertionError("no seed in 1..20 is insensitive at every step")


def _device_run(model, seed, n, prompt, monkeypatch):
    def no_torch_path(self, logits, coin=None):
        raise AssertionError("the host sample_torch path was taken")
    with monkeypatch.context() as mp:
        mp.setattr(Sampler, "sample_torch", no_torch_path)
        out, _ = InferenceEngine(model, sampler=Sampler(256, T, TOPP, seed)) \
            .generate(prompt, n)
    return out


def test_generate_matches_host_sampling(tiny, monkeypatch):
    base = _model(tiny, False)
    base.capture_decode_graph()
    seed, want = _baseline(base, 24, [3, 17, 101])
    dev = _model(tiny, True)
    dev.capture_decode_graph()
    assert dev._graph_samples and not base._graph_samples
    assert _device_run(dev, seed, 24, [3, 17, 101], monkeypatch) == want


def test_tp_path_world1_matches_plain(tiny, monkeypatch):
    plain = _model(tiny, False)
    plain.capture_decode_graph()
    seed, want = _baseline(plain, 12, [3, 17, 101])
    tp = _model(tiny, True, force_sync=True)
    tp.capture_decode_graph()
    assert tp._graph_samples and tp.tp_path
    assert _device_run(tp, seed, 12, [3, 17, 101], monkeypatch) == want


def test_split_recapture_keeps_the_sampler(tiny):
    """Crossing the adaptive K-split threshold recaptures the decode graph;
    the new graph must still end in the sampler."""
    model = _model(tiny, True)
    model.adaptive_thresh = 6
    model.forward(torch.tensor([3, 17, 101]), torch.arange(3))
    model.capture_decode_graph()
    graph = model._graph
    coins = Sampler(256, T, TOPP, 99)
    token = 7
    for i in range(6):  # positions 3..8 cross the threshold at 6
        coin = coins.next_coin()
        got = model.forward_sample(torch.tensor([token]), torch.tensor([3 + i]),
                                   coin, T, TOPP)
        want = model.sample_row(model.last_logits().clone(), coin, T, TOPP)
        assert got == want and got is not None, i
        token = got
    assert model.attn_splits == 16 and model._graph is not graph
    assert model._graph_samples


def test_forward_sample_without_a_sampling_graph(tiny):
    """--no-graph, and a graph captured before device_sampling was set: the
    step runs as it would for forward, the sampler launches follow it."""
    eager = _model(tiny, True)
    late = _model(tiny, False)
    ref = _model(tiny, False)
    for m in (eager, late, ref):
        m.forward(torch.tensor([3, 17, 101]), torch.arange(3))
    late.capture_decode_graph()
    late.device_sampling = True
    assert late._graph is not None and not late._graph_samples
    for i, (temp, topp) in enumerate([(0.8, 0.9), (0.0, 0.9), (1.2, 1.0)]):
        coin = (i + 0.5) / 3
        t, p = torch.tensor([7 + 13 * i]), torch.tensor([3 + i])
        row = ref.forward(t, p)[0]
        for m in (eager, late):
            got = m.forward_sample(t, p, coin, temp, topp)
            # the step ran (same logits as a plain forward, up to the order
            # of its float atomics) and the sampler ran over its row
            assert _rel_err(m.last_logits(), row) < 1e-4
            assert got == m.sample_row(m.last_logits().clone(), coin, temp, topp)
            assert got is not None
