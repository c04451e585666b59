"""row_runs: the runs of a row step's slots list."""

import pytest

from dllama_amd.models.rows import row_runs

CASES = {
    "all decode": ([3, 0, 2, 1], [(0, 1), (1, 1), (2, 1), (3, 1)]),
    "one chunk": ([1] * 32, [(0, 32)]),
    "decode then chunk": ([0, 2] + [1] * 9, [(0, 1), (1, 1), (2, 9)]),
    "40 rows cut at 32": ([4] * 40, [(0, 32), (32, 8)]),
    "alternating": ([0, 1, 0, 1], [(0, 1), (1, 1), (2, 1), (3, 1)]),
    "one row": ([5], [(0, 1)]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_row_runs(name):
    slots, want = CASES[name]
    assert row_runs(slots) == want
