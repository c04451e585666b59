"""Host side of the on-device sampler: the Sampler split into next_coin +
sample_with_coin, the float64 oracle sample_ref, and the engine hook that
hands the coin to a model that samples on device."""

import numpy as np
import pytest
import torch

from dllama_amd.engine import InferenceEngine
from dllama_amd.ops.reference import sample_ref
from dllama_amd.tokenizer import Sampler, _xorshift_u32

V = 1000
SEEDS = (1, 12345, 2 ** 40 + 3)
TOPPS = (0.9, 1.0, 0.0)


def _logits(n=50, v=V, seed=0):
    return (np.random.default_rng(seed).standard_normal((n, v)) * 3).astype(np.float32)


def _coins(seed, n):
    """The xorshift stream of a seed, computed apart from the Sampler."""
    state, out = seed, []
    for _ in range(n):
        u, state = _xorshift_u32(state)
        out.append((u >> 8) / 16777216.0)
    return out, state


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("topp", TOPPS)
def test_sample_equals_coin_then_sample_with_coin(seed, topp):
    rows = _logits()
    a = Sampler(V, 0.8, topp, seed)
    b = Sampler(V, 0.8, topp, seed)
    coins, state = _coins(seed, len(rows))
    for row, want_coin in zip(rows, coins):
        coin = b.next_coin()
        assert coin == want_coin
        assert a.sample(row) == b.sample_with_coin(row, coin)
    assert a.state == b.state == state


@pytest.mark.parametrize("seed", SEEDS)
def test_greedy_draws_no_coin(seed):
    rows = _logits(5)
    s = Sampler(V, 0.0, 0.9, seed)
    for row in rows:
        assert s.sample(row) == int(np.argmax(row))
        assert s.sample_with_coin(row, None) == int(np.argmax(row))
    assert s.state == seed


@pytest.mark.parametrize("topp", TOPPS)
def test_sample_ref_agrees_outside_margin(topp):
    rows = _logits(seed=1)
    s = Sampler(V, 0.8, topp, 12345)
    judged = 0
    for row in rows:
        coin = s.next_coin()
        tok, margin = sample_ref(row, 0.8, topp, coin)
        if margin >= 1e-5:
            judged += 1
            assert tok == s.sample_with_coin(row, coin)
    assert judged >= 45


def test_sample_ref_known_probabilities():
    # p = 0.1, 0.4, 0.2, 0.3; descending order: 1, 3, 2, 0
    logits = np.log(np.array([0.1, 0.4, 0.2, 0.3]))
    # cutoff (1 - 0.75) / 3 keeps all four; c = .4 .7 .9 1.0, last = 2 (.9 > .75)
    for coin, want in ((0.0, 1), (0.2, 1), (0.5, 3), (0.7, 3), (0.8, 2), (0.99, 2)):
        tok, margin = sample_ref(logits, 1.0, 0.75, coin)
        assert tok == want, (coin, tok)
        assert margin > 1e-3
    # a nucleus of one: c[0] = .4 > .3
    assert sample_ref(logits, 1.0, 0.3, 0.999)[0] == 1
    # multinomial walks the vocabulary order: cdf = .1 .5 .7 1.0
    for topp in (0.0, 1.0):
        for coin, want in ((0.05, 0), (0.3, 1), (0.6, 2), (0.95, 3)):
            tok, margin = sample_ref(logits, 1.0, topp, coin)
            assert tok == want
            assert margin > 0.04
    # temperature sharpens: T = 0.5 squares the odds, p = 1 16 4 9 / 30
    assert sample_ref(logits, 0.5, 1.0, 0.5)[0] == 1
    assert sample_ref(logits, 0.5, 1.0, 0.6)[0] == 2
    assert sample_ref(logits, 0.0, 0.9, 0.3) == (1, float("inf"))


def test_sample_ref_all_equal():
    logits = np.full(64, 1.5, dtype=np.float32)
    # every token is a candidate, ties keep the index order; c_j = (j+1)/64
    # and the first c > 0.9 is j = 57, so r = coin * 58/64
    for j in (0, 1, 30, 57):
        tok, margin = sample_ref(logits, 0.8, 0.9, (j + 0.5) / 58)
        assert tok == j
        assert margin > 1e-3
    assert sample_ref(logits, 0.8, 0.9, (2 ** 24 - 1) / 2 ** 24)[0] == 57
    assert sample_ref(logits, 0.8, 1.0, 10.5 / 64)[0] == 10
    assert sample_ref(logits, 0.0, 0.9, 0.5)[0] == 0


# ------------------------------------------------------------ engine hook

class _Cfg:
    seq_len = 64


class _HostModel:
    """No device sampler: forward returns scripted logits rows."""

    cfg = _Cfg()

    def __init__(self, rows):
        self.rows = torch.from_numpy(rows)
        self.step = 0
        self.skip_logits = False

    def forward(self, tokens, positions):
        n = tokens.shape[0]
        self.step += 1
        return self.rows[self.step - 1].repeat(n, 1)


class _DeviceModel(_HostModel):
    """Offers the device sampling hook: records its arguments and answers
    from a script (None = the device sampler gave up)."""

    def __init__(self, rows, script):
        super().__init__(rows)
        self.script = list(script)
        self.calls = []

    def _answer(self, kind, coin, temperature, topp):
        self.calls.append((kind, coin, temperature, topp))
        return self.script[len(self.calls) - 1]

    def sample_row(self, row, coin, temperature, topp):
        assert torch.equal(row, self.rows[self.step - 1])
        return self._answer("row", coin, temperature, topp)

    def forward_sample(self, tokens, positions, coin, temperature, topp):
        self.forward(tokens, positions)
        self.fed = int(tokens[0])
        return self._answer("step", coin, temperature, topp)

    def last_logits(self):
        return self.rows[self.step - 1]


def test_engine_passes_the_coin_stream_to_the_device_sampler():
    seed, n = 12345, 6
    rows = _logits(n, seed=2)
    script = [11, 22, None, 44, 55, 66]
    model = _DeviceModel(rows, script)
    sampler = Sampler(V, 0.8, 0.9, seed)
    eng = InferenceEngine(model, sampler=sampler)
    out, _ = eng.generate([1, 2, 3], n)
    coins, state = _coins(seed, n)
    assert [c[0] for c in model.calls] == ["row"] + ["step"] * (n - 1)
    assert [c[1] for c in model.calls] == coins
    assert all(c[2:] == (0.8, 0.9) for c in model.calls)
    assert sampler.state == state
    # the None step is resampled on the host path with the same coin
    want = Sampler(V, 0.8, 0.9, 1).sample_with_coin(rows[2], coins[2])
    assert out == [11, 22, want, 44, 55, 66]
    assert model.fed == 55 and eng.pos == 3 + n - 1


def test_engine_follows_sampler_changes_and_draws_no_coin_when_greedy():
    rows = _logits(4, seed=3)
    model = _DeviceModel(rows, [5, 6, 7, 8])
    sampler = Sampler(V, 0.0, 0.5, 777)
    out, _ = InferenceEngine(model, sampler=sampler).generate([9], 4)
    assert out == [5, 6, 7, 8]
    assert sampler.state == 777
    assert all(c[1:] == (0.0, 0.0, 0.5) for c in model.calls)
    # first token given up by the device sampler
    model = _DeviceModel(rows, [None, 6])
    sampler = Sampler(V, 1.3, 1.0, 777)
    out, _ = InferenceEngine(model, sampler=sampler).generate([9], 2)
    coins, _ = _coins(777, 2)
    assert out == [Sampler(V, 1.3, 1.0, 1).sample_with_coin(rows[0], coins[0]), 6]
    assert [c[1:] for c in model.calls] == [(coins[0], 1.3, 1.0), (coins[1], 1.3, 1.0)]


def test_engine_keeps_host_path_without_the_hook():
    seed, n = 4242, 5
    rows = _logits(n, seed=4)
    ref = Sampler(V, 0.8, 0.9, seed)
    want = [ref.sample(r) for r in rows]
    sampler = Sampler(V, 0.8, 0.9, seed)
    out, _ = InferenceEngine(_HostModel(rows), sampler=sampler).generate([1], n)
    assert out == want and sampler.state == ref.state
    # a model that has the methods but switched them off is a host model too
    model = _DeviceModel(rows, [])
    model.device_sampling = False
    sampler = Sampler(V, 0.8, 0.9, seed)
    out, _ = InferenceEngine(model, sampler=sampler).generate([1], n)
    assert out == want and model.calls == []
