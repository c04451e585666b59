"""Ragged steps: the per-row {slot, position} table shared by the models.

A step of B rows carries, for every row, a token, the KV slot of its
sequence and its position inside that sequence. One table expresses N
sequences decoding together, a prompt chunk into any slot, and a mix.
"""

from __future__ import annotations


def as_ints(v) -> list[int]:
    """A list of Python ints from a list, tuple or integer tensor."""
    if hasattr(v, "tolist"):
        v = v.tolist()
    return [int(x) for x in v]


def check_rows(tokens, slots, positions, n_slots: int, seq_len: int,
               n_batches: int) -> tuple[list[int], list[int], list[int]]:
    """Validate one ragged step; returns (tokens, slots, positions) as int
    lists. Raises ValueError before anything runs: the kernels index the KV
    cache with these values unchecked."""
    tokens, slots, positions = as_ints(tokens), as_ints(slots), as_ints(positions)
    B = len(tokens)
    if B < 1 or len(slots) != B or len(positions) != B:
        raise ValueError(
            f"a row step needs equally many tokens, slots and positions "
            f"(got {B}, {len(slots)}, {len(positions)}), and at least one")
    if B > n_batches:
        raise ValueError(f"{B} rows exceed n_batches {n_batches}")
    seen = set()
    for s, p in zip(slots, positions):
        if not 0 <= s < n_slots:
            raise ValueError(f"slot {s} outside the model's {n_slots} KV slots")
        if not 0 <= p < seq_len:
            raise ValueError(
                f"position {p} exceeds seq_len {seq_len} "
                "(rebuild with a larger --max-seq-len / seq_len)")
        if (s, p) in seen:
            raise ValueError(f"two rows address slot {s} position {p}")
        seen.add((s, p))
    return tokens, slots, positions


def is_decode_step(slots: list[int]) -> bool:
    """Every row belongs to another sequence: one decode row each."""
    return len(set(slots)) == len(slots)
