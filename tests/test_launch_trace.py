"""The kernel launch sequences of `HipTransformer` are pinned.

`tools/launch_trace.py` replays a matrix of architectures, sync modes and
env-gated options on the CPU, with recorders in place of the HIP extension
and the communicator, and these tests compare every `(kernel, args)` list
with a golden: the single-sequence step `forward_buffers` over batch sizes
with `tests/golden/launch_trace.json`, and row steps (`forward_rows`, by
row table and by row table plus page table) with
`tests/golden/launch_trace_rows.json`. A restructuring of the model code
that launches another kernel, passes another weight, `ssq` slot or slice,
or reorders two launches fails here, on a box without a GPU. The first
golden also pins the weights that `synthetic` draws, so outputs dumped by
the benchmark stay comparable across commits."""

import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), "tools"))


def test_launch_traces_match_golden():
    import launch_trace as lt
    with open(lt.GOLDEN) as f:
        gold = json.load(f)
    # every configuration of the matrix runs: one that raises fails the test
    live, live_calls = lt.build_live()
    assert len(live["configs"]) == len(list(lt.configs())) > 150
    assert all(len(ids) == len(lt.BATCHES) * len(lt.MODES)
               for ids in live["configs"].values())
    assert all(len(live["traces"][i]) >= 5
               for ids in live["configs"].values() for i in ids)
    errs = lt.compare(gold, live, live_calls)
    assert not errs, f"{len(errs)} mismatches, first:\n" + "\n".join(errs[:3])


def test_row_step_launch_traces_match_golden():
    import launch_trace as lt
    with open(lt.GOLDEN_ROWS) as f:
        gold = json.load(f)
    live, live_calls = lt.build_live(lt.ROWS)
    assert (len(live["configs"])
            == len(list(lt.configs())) * len(lt.ADDRESSINGS) > 300)
    assert all(len(ids) == len(lt.ROW_STEPS) * len(lt.ROW_MODES)
               for ids in live["configs"].values())
    assert all(len(live["traces"][i]) >= 5
               for ids in live["configs"].values() for i in ids)
    # a mismatch names "<arch>/<sync>/<env>/<addressing> step=<step>
    # greedy_feedback=... skip_logits=..."
    errs = lt.compare(gold, live, live_calls, lt.ROWS)
    assert not errs, f"{len(errs)} mismatches, first:\n" + "\n".join(errs[:3])


def test_golden_is_small():
    import launch_trace as lt
    for path in (lt.GOLDEN, lt.GOLDEN_ROWS):
        assert os.path.getsize(path) < 200 * 1024
