"""prefix_groups (models/rows.py) on hand-written page lists: which decode
rows of a step share a run of leading pages, and how long it is."""

import pytest

from dllama_amd.models.rows import prefix_groups

P = 16
U = -1  # an unmapped table entry


def groups(page_rows, positions=None, cols=32, min_rows=2, min_tokens=0):
    positions = positions or [500] * len(page_rows)
    return prefix_groups(page_rows, positions, P, cols, min_rows, min_tokens)


@pytest.mark.parametrize("page_rows,kw,want", [
    # a common prefix of two pages, each row with pages of its own behind it
    ([[4, 9, 1, U], [4, 9, 7, 2], [4, 9, 3, U]], {}, [([0, 1, 2], 2 * P)]),
    # the common run of a bucket is its first page only
    ([[4, 9, 1], [4, 8, 1], [4, 9, 1]], {}, [([0, 1, 2], P)]),
    # two buckets, rows interleaved: groups in the order of their first rows
    ([[5, 6], [4, 9], [5, 6, 2], [4, 9, 3], [8, 1]], {},
     [([0, 2], 2 * P), ([1, 3], 2 * P)]),
    # min_tokens: a prefix of 32 tokens does not reach 33, and reaches 32
    ([[4, 9, 1], [4, 9, 2]], dict(min_tokens=2 * P + 1), []),
    ([[4, 9, 1], [4, 9, 2]], dict(min_tokens=2 * P), [([0, 1], 2 * P)]),
    # min_rows: a bucket of two is too small for 3
    ([[4, 9, 1], [4, 9, 2], [7]], dict(min_rows=3), []),
    # cols_per_group: five rows cut 2 + 2 + 1, the rest a group of its own
    ([[4, 1], [4, 2], [4, 3], [4, 5], [4, 6]], dict(cols=2),
     [([0, 1], P), ([2, 3], P), ([4], P)]),
    # min_rows counts the bucket, not its cuts: 4 rows qualify for 4 and are
    # cut at 2 columns; 3 rows do not qualify
    ([[4, 1], [4, 2], [4, 3], [4, 5]], dict(cols=2, min_rows=4),
     [([0, 1], P), ([2, 3], P)]),
    ([[4, 1], [4, 2], [4, 3]], dict(cols=2, min_rows=4), []),
    # unmapped entries: they end the run, a row without pages joins nothing,
    # and neither does a row that is no decode row (None)
    ([[4, 9, U, U], [4, 9, U, U], [U, U, U, U], None, [4, 9, 3, U]], {},
     [([0, 1, 4], 2 * P)]),
    ([[4, U, 6], [4, U, 6]], {}, [([0, 1], P)]),
], ids=["common", "one-page", "order", "min-tokens-below", "min-tokens-at",
        "min-rows", "cut", "min-rows-above-cols", "min-rows-above-cols-short",
        "unmapped", "unmapped-hole"])
def test_prefix_groups(page_rows, kw, want):
    assert groups(page_rows, **kw) == want
    assert groups(page_rows, **kw) == want  # the same again: no hidden state


def test_prefix_lies_below_every_position():
    """A shared page is full and read-only: a member inside it is a broken
    step, not a group."""
    with pytest.raises(AssertionError):
        groups([[4, 9, 1], [4, 9, 2]], positions=[40, 31])
