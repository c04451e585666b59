"""When `HipTransformer` captures, replays and drops its step graphs.

No GPU: the model is the recorder model of `tools/launch_trace.py` (llama64
on the CPU, the kernels record their launches and run nothing), and its
graph store gets a fake capture function. The fake runs the body
`warmups + 1` times and the tail once, as a capture does; the object it
returns appends "replay" to an event list when replayed and, for a decode
graph, advances `model.pos` as the captured `pos_inc` would. Every capture
attempt appends `(key, attn_splits)` to the same list.
"""

import os
import sys
from unittest import mock

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), "tools"))

import launch_trace as lt  # noqa: E402
from dllama_amd.models.graphs import StepGraphs  # noqa: E402

DEC_OFF, DEC_ON = ("decode", False), ("decode", True)


class SamplingKernels(lt.RecordingKernels):
    """The recorder, answering the three questions whose answers size the
    sampler's and the log-probability scratch."""

    def sampler_blocks(self, vocab):
        return 2

    def sampler_max_candidates(self):
        return 8

    def logprob_chunks(self, vocab):
        return 2


@pytest.fixture(scope="module")
def llama64(tmp_path_factory):
    return lt.write_models(str(tmp_path_factory.mktemp("models")))["llama64"]


class Harness:
    """A recorder model whose store captures with the fake."""

    def __init__(self, path, **ctor):
        with mock.patch.object(lt, "RecordingKernels", SamplingKernels):
            self.model, self.kernels, content = lt._recorded_model(
                path, "llama64", "plain", "none", **ctor)
        self.kernels.trace = lt.Trace(content)
        self.events = []
        self.failing = False
        model, events, harness = self.model, self.events, self

        class FakeGraph:
            key = None

            def replay(self):
                events.append("replay")
                if self.key[0] == "decode":
                    model.pos += 1

        def capture(body, warmups, tail=None):
            if harness.failing:
                raise RuntimeError("capture is not supported here")
            for _ in range(warmups + 1):
                body()
            if tail is not None:
                tail()
            return FakeGraph()

        class Recording(StepGraphs):
            def capture(self, key, plan):
                events.append((key, model.attn_splits))
                g = super().capture(key, plan)
                g.key = key
                return g

        model.graphs = Recording(capture, on_gpu=True)

    def captures(self, since=0):
        return [e for e in self.events[since:] if e != "replay"]

    def replays(self, since=0):
        return self.events[since:].count("replay")

    def launches(self):
        """Kernel launches since the last call: an eager step has some, a
        replay of a fake graph has none."""
        n = len(self.kernels.trace.calls)
        self.kernels.trace.calls.clear()
        return n

    def decode(self, p0, sample=False):
        t, p = torch.tensor([7]), torch.tensor([p0])
        if sample:
            return self.model.forward_sample(t, p, 0.3, 0.8, 0.9)
        return self.model.forward(t, p)

    def prompt(self, n=3, at=0):
        self.model.forward(torch.arange(5, 5 + n), torch.arange(at, at + n))


def _tiers(model):
    """S=1 below position 4, S=8 below 8, S=16 from 8 on."""
    model.wide_thresh, model.adaptive_thresh = 4, 8


# ------------------------------------------------------------ 1: decode

def test_decode_graph_follows_the_split_count(llama64):
    h = Harness(llama64)
    model, c = h.model, h.model.cfg
    _tiers(model)
    h.prompt(3)
    model.capture_decode_graph()
    assert h.captures() == [(DEC_OFF, 1)]  # the prompt left the wide tier on
    fills = []
    fill = torch.Tensor.fill_

    def counting_fill(t, value):
        if t is model.pos:
            fills.append(value)
        return fill(t, value)

    written = {}
    h.launches()
    with mock.patch.object(torch.Tensor, "fill_", counting_fill):
        for p0 in range(3, 10):
            stale = model._graph_pos != p0
            seen, n = len(h.events), len(fills)
            h.decode(p0)
            want_s = 1 if p0 < 4 else 8 if p0 < 8 else 16
            # a capture only at the step that first needs the split count
            assert h.captures(seen) == (
                [(DEC_OFF, want_s)] if p0 in (4, 8) else [])
            # one replay; only the fake capture's body runs launch anything
            assert h.replays(seen) == 1
            assert (h.launches() > 0) == (p0 in (4, 8))
            assert model.attn_splits == want_s
            n_split = model.n_batches * c.n_heads0 * want_s
            assert model.attn_ml.numel() == 2 * n_split
            assert model.attn_o.numel() == n_split * c.head_dim
            # the host writes pos where the graph did not leave it, at most
            # once more around a capture, and at no other step
            written[p0] = len(fills) - n
            assert int(stale) <= written[p0] <= int(stale or p0 in (4, 8))
            assert int(model.pos) == p0 + 1 == model._graph_pos
    assert written[3] == 1
    assert not any(written[p] for p in (5, 6, 7, 9))
    assert len(h.captures()) == 3 and h.replays() == 7

    # a prompt chunk between two decode steps takes the position away and
    # captures nothing for decode
    seen = len(h.events)
    h.prompt(5, at=10)
    assert model._graph_pos is None and h.events[seen:] == []
    h.decode(15)
    assert h.events[seen:] == ["replay"] and int(model.pos) == 16


# ------------------------------------------------------------ 2: logprobs

def test_graphs_of_both_logprob_settings(llama64):
    """The sequence of test_logprob_model's
    test_graphs_of_both_settings_are_kept, through both entry points."""
    h = Harness(llama64)
    model = h.model
    model.device_sampling = True
    h.prompt(3)
    model.capture_decode_graph()
    g_off = model._graph
    assert g_off is not None and model._graph_samples
    h.decode(3, sample=True)
    h.decode(4)
    model.set_logprobs(True)
    assert model._graph is None and h.captures() == [(DEC_OFF, 1)]
    h.decode(5, sample=True)
    g_on = model._graph
    assert g_on is not None and g_on is not g_off and model._graph_samples
    assert h.captures() == [(DEC_OFF, 1), (DEC_ON, 1)]
    # toggling recaptures nothing
    seen = len(h.events)
    model.set_logprobs(False)
    assert model._graph is g_off and model._graph_samples
    h.decode(6, sample=True)
    assert model._graph is g_off
    model.set_logprobs(True)
    assert model._graph is g_on
    h.decode(7)
    assert h.events[seen:] == ["replay", "replay"]
    # a split change drops the graphs of both settings ...
    model._set_attn_splits(16)
    assert model._graph is not g_on
    model.set_logprobs(False)
    assert model._graph is None
    # ... and each comes back only at the next step of its own setting
    seen = len(h.events)
    assert h.decode(8, sample=True) is not None
    assert model._graph is not None and model._graph is not g_off
    assert {key for key, _ in h.captures(seen)} == {DEC_OFF}
    assert h.events[-2:] == [(DEC_OFF, 1), "replay"] and h.replays(seen) == 1
    h.decode(9)
    model.set_logprobs(True)
    assert model._graph is None
    h.decode(10)
    assert model._graph is not None and model._graph is not g_on
    assert h.replays(seen) == 3
    # lazily: one capture per setting since the split change, none at the
    # change itself (before the store there was one more)
    assert h.captures(seen) == [(DEC_OFF, 1), (DEC_ON, 1)]


def test_graph_from_before_device_sampling_stays(llama64):
    h = Harness(llama64)
    model = h.model
    h.prompt(3)
    model.capture_decode_graph()
    model.device_sampling = True
    graph = model._graph
    h.launches()
    h.decode(3, sample=True)
    assert model._graph is graph and not model._graph_samples
    # one replay, then the sampler eagerly
    assert h.events[-1] == "replay" and h.launches() == 1


# ------------------------------------------------------------ 3: failure

def test_failed_decode_capture_means_eager(llama64, capsys):
    h = Harness(llama64)
    model = h.model
    _tiers(model)
    h.prompt(3)
    h.failing = True
    with pytest.raises(RuntimeError):
        model.capture_decode_graph()
    assert model._graph is None and len(h.captures()) == 1
    h.launches()
    for p0 in range(3, 13):
        h.decode(p0)
        assert h.launches() > 0  # ran eager
    assert len(h.captures()) == 1 and h.replays() == 0
    assert model._graph is None


def test_failed_recapture_at_a_split_change(llama64):
    h = Harness(llama64)
    model = h.model
    _tiers(model)
    h.prompt(3)
    model.capture_decode_graph()
    h.decode(3)
    assert h.events == [(DEC_OFF, 1), "replay"]
    h.failing = True
    h.launches()
    seen = len(h.events)
    for p0 in range(4, 14):
        h.decode(p0)
        assert h.launches() > 0
    # one attempt at the first step past the tier; the graph of the old
    # split count is gone and nothing is replayed
    assert h.events[seen:] == [(DEC_OFF, 8)]
    assert model._graph is None


# ------------------------------------------------------------ 4: prefill

def _chunk(h, at=0):
    h.model.forward(torch.arange(32), torch.arange(at, at + 32))


def test_prefill_graph_per_skip_logits(llama64):
    h = Harness(llama64)
    model = h.model
    model.wide_thresh = 0  # no wide tier: a chunk leaves the split count be
    S = model.attn_splits
    _chunk(h)
    assert h.events == [(("prefill", False), S), "replay"]
    _chunk(h, 32)
    assert h.events[2:] == ["replay"]
    model.skip_logits = True
    _chunk(h)
    _chunk(h)
    assert h.events[3:] == [(("prefill", True), S), "replay", "replay"]
    assert model.skip_logits is True
    model.skip_logits = False
    seen = len(h.events)
    _chunk(h)
    assert h.events[seen:] == ["replay"]
    # a split change drops them
    model._set_attn_splits(16)
    seen = len(h.events)
    _chunk(h)
    _chunk(h)
    assert h.events[seen:] == [(("prefill", False), 16), "replay", "replay"]


def test_failed_prefill_capture_is_silent_and_final(llama64, capsys):
    h = Harness(llama64)
    h.failing = True
    _chunk(h)
    assert len(h.captures()) == 1 and h.launches() > 0  # eager, same call
    h.failing = False
    _chunk(h, 32)
    h.model._set_attn_splits(16)
    h.model.skip_logits = True
    _chunk(h)
    assert len(h.captures()) == 1 and h.replays() == 0 and h.launches() > 0
    out = capsys.readouterr()
    assert out.out == "" and out.err == ""


# ------------------------------------------------------------ 5: rows

def _rows_harness(path, addressing):
    ctor, pages = lt.ADDRESSINGS[addressing]
    h = Harness(path, **ctor)
    for slot, ids in pages.items():
        h.model.set_slot_pages(slot, ids)
    return h


def _rows_step(h, step, sample=True):
    """All-decode step number `step` of three sequences."""
    tokens, slots, positions = lt.ROW_STEPS["all_decode"]
    positions = [p + step for p in positions]
    if not sample:
        return h.model.forward_rows(tokens, slots, positions)
    return h.model.forward_rows_sample(tokens, slots, positions, [0.5] * 3,
                                       [0.8] * 3, [0.9] * 3)


@pytest.mark.parametrize("addressing", ["table", "paged"])
def test_row_graphs(llama64, addressing):
    h = _rows_harness(llama64, addressing)
    model = h.model
    ROWS_OFF, ROWS_ON = ("rows", 3, False), ("rows", 3, True)
    assert _rows_step(h, 0) == [0, 0, 0]
    S = model.attn_splits
    assert h.events == [(ROWS_OFF, S), "replay"]
    # the graph's table advance is booked: the second step finds its table
    # on the device
    dev = list(model._rows_dev)
    assert [p for _, p in dev] == [4, 10, 21]
    _rows_step(h, 1)
    assert h.events[2:] == ["replay"]
    assert model._rows_dev == [(base, p + 1) for base, p in dev]
    g_off = model._row_graphs[3]
    assert list(model._row_graphs) == [3]
    # a step with a prompt chunk in it runs eager
    h.launches()
    model.forward_rows(*lt.ROW_STEPS["mixed"])
    assert h.events[3:] == [] and h.launches() > 0
    # the other set_logprobs setting has a graph of its own
    model.set_logprobs(True)
    assert not model._row_graphs and model._row_graphs.get(3) is None
    _rows_step(h, 2)
    assert h.events[3:] == [(ROWS_ON, S), "replay"]
    assert list(model._row_graphs) == [3]
    g_on = model._row_graphs[3]
    assert g_on is not g_off and 3 in model._row_graphs
    model.set_logprobs(False)
    assert model._row_graphs[3] is g_off
    _rows_step(h, 3, sample=False)
    assert h.events[5:] == ["replay"]


def test_row_graphs_switched_off(llama64):
    h = _rows_harness(llama64, "table")
    h.model.row_graphs = False
    _rows_step(h, 0)
    _rows_step(h, 1)
    assert h.events == [] and not h.model._row_graphs and h.launches() > 0


def test_failed_row_capture_warns_once(llama64, capsys):
    h = _rows_harness(llama64, "table")
    h.failing = True
    for step in range(3):
        h.launches()
        _rows_step(h, step)
        assert h.launches() > 0
    h.failing = False
    _rows_step(h, 3)
    assert len(h.captures()) == 1 and h.replays() == 0
    err = capsys.readouterr().err
    assert err.count("row-step graph capture failed") == 1
    assert err.count("\n") == 1


def test_model_is_freed_without_the_garbage_collector(llama64):
    """The store must not refer back to its model: a dropped model in a
    reference cycle, with the graphs it holds, would be freed by whichever
    collection comes next, possibly in the middle of another model's
    capture, where releasing a graph aborts the process."""
    import gc
    import weakref
    gc.collect()
    gc.disable()
    try:
        model, kernels, content = lt._recorded_model(
            llama64, "llama64", "plain", "none")
        kernels.trace = lt.Trace(content)
        model.forward(torch.arange(3), torch.arange(3))
        ref = weakref.ref(model)
        del model
        assert ref() is None
    finally:
        gc.enable()


# ------------------------------------------------------------ 6: the store

def _plan(note=None):
    return lambda: (lambda: None, 1, None, note)


def test_store_alone():
    made = []

    def capture(body, warmups, tail=None):
        made.append(object())
        return made[-1]

    store = StepGraphs(capture, on_gpu=True)
    assert store.get(DEC_OFF) is None  # nothing to capture from
    g = store.get(DEC_OFF, _plan(True))
    assert g is made[0] and store.entries[DEC_OFF] == (g, True)
    assert store.get(DEC_OFF, _plan()) is g and len(made) == 1
    assert store.get(DEC_ON) is None
    rows = store.get(("rows", 3, False), _plan())
    assert store.get(("rows", 3, True)) is None
    assert store.get(("rows", 4, False)) is None
    assert store.entries == {DEC_OFF: (g, True),
                             ("rows", 3, False): (rows, None)}
    # an explicit capture replaces what was there
    assert store.capture(DEC_OFF, _plan(False)) is made[-1] is not g
    assert store.entries[DEC_OFF] == (made[-1], False)
    store.clear()
    assert store.entries == {} and store.get(DEC_OFF) is None


def test_store_allowed_and_failure_memory():
    def capture(body, warmups, tail=None):
        raise RuntimeError("no")

    made = []
    store = StepGraphs(lambda *step: made.append(1) or object(), on_gpu=True)
    assert store.allowed("rows") and not store.allowed("rows", enabled=False)
    assert store.get(("rows", 3, False), _plan(), enabled=False) is None
    assert not made
    assert not StepGraphs(None, on_gpu=False).allowed("decode")
    assert StepGraphs(None, on_gpu=False).get(DEC_OFF, _plan()) is None

    assert store.get(("prefill", True), _plan()) is not None
    store._capture = capture
    errors = []
    assert store.get(("prefill", False), _plan(),
                     on_error=errors.append) is None
    assert len(errors) == 1 and store.failed == {"prefill"}
    # the kind is eager from now on: no graph, no new attempt, no report
    assert store.get(("prefill", True), _plan()) is None
    assert store.get(("prefill", False), _plan(),
                     on_error=errors.append) is None
    assert len(errors) == 1 and not store.allowed("prefill")
    # ... also after the graphs were dropped; other kinds are not touched
    store.clear()
    assert store.failed == {"prefill"} and store.allowed("decode")
    # capture() itself raises, having remembered the failure
    with pytest.raises(RuntimeError):
        store.capture(DEC_OFF, _plan())
    assert store.failed == {"prefill", "decode"}
    assert store.get(DEC_OFF, _plan()) is None
