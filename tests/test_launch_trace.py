"""The kernel launch sequence of `HipTransformer.forward_buffers` is pinned.

`tools/launch_trace.py` replays a matrix of architectures, sync modes,
batch sizes and env-gated options on the CPU, with recorders in place of
the HIP extension and the communicator, and this test compares every
`(kernel, args)` list with `tests/golden/launch_trace.json`. A restructuring
of the model code that launches another kernel, passes another weight,
`ssq` slot or slice, or reorders two launches fails here, on a box without
a GPU. The golden also pins the weights that `synthetic` draws, so outputs
dumped by the benchmark stay comparable across commits."""

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


def test_golden_is_small():
    import launch_trace as lt
    assert os.path.getsize(lt.GOLDEN) < 200 * 1024
