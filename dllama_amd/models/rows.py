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


PAGE_SIZES = (4, 8, 16, 32, 64, 128, 256)


class PageMap:
    """Host side of a paged model's page table: which pool page holds each
    page index of every slot (-1 = unmapped), and how many table entries
    name each page. The models keep their device (or gather) view in step
    with it; check() is what stands between a row step and the kernels,
    which follow the table unchecked."""

    def __init__(self, n_slots: int, seq_len: int, kv_pages: int,
                 page_size: int):
        if page_size not in PAGE_SIZES:
            raise ValueError(
                f"page_size must be a power of two in 4..256 (got {page_size})")
        if kv_pages < 1:
            raise ValueError(f"kv_pages must be >= 1 (got {kv_pages})")
        self.n_slots = n_slots
        self.kv_pages = kv_pages
        self.page_size = page_size
        self.pages_per_seq = -(-seq_len // page_size)
        self.table = [[-1] * self.pages_per_seq for _ in range(n_slots)]
        self.users = [0] * kv_pages
        self._lead = [0] * n_slots  # mapped pages at the start of each slot
        self.dirty: set[int] = set()  # slots whose mapping the view lacks

    def _slot(self, slot: int) -> list[int]:
        if not 0 <= slot < self.n_slots:
            raise ValueError(
                f"slot {slot} outside the model's {self.n_slots} KV slots")
        return self.table[slot]

    def set_slot_pages(self, slot: int, pages, first: int = 0) -> None:
        """Map pages into the slot's table from page index `first`."""
        row = self._slot(slot)
        pages = as_ints(pages)
        if first < 0 or first + len(pages) > self.pages_per_seq:
            raise ValueError(
                f"pages {first}..{first + len(pages) - 1} outside the "
                f"{self.pages_per_seq} pages of a sequence")
        for p in pages:
            if not 0 <= p < self.kv_pages:
                raise ValueError(
                    f"page {p} outside the pool's {self.kv_pages} pages")
        for i, p in enumerate(pages, first):
            if row[i] >= 0:
                self.users[row[i]] -= 1
            row[i] = p
            self.users[p] += 1
        self._touched(slot)

    def clear_slot(self, slot: int) -> None:
        row = self._slot(slot)
        for i, p in enumerate(row):
            if p >= 0:
                self.users[p] -= 1
                row[i] = -1
        self._touched(slot)

    def _touched(self, slot: int) -> None:
        row = self.table[slot]
        n = 0
        while n < len(row) and row[n] >= 0:
            n += 1
        self._lead[slot] = n
        self.dirty.add(slot)

    def device_row(self, slot: int) -> list[int]:
        """The slot's table as the device holds it: unmapped entries are 0,
        so no entry ever points outside the pool."""
        return [max(p, 0) for p in self.table[slot]]

    def cache_row(self, slot: int, pos: int) -> int:
        P = self.page_size
        return self.table[slot][pos // P] * P + pos % P

    def check(self, slots: list[int], positions: list[int]) -> None:
        """ValueError for a row whose position lies in an unmapped page or
        above one, and for a row that would write its K/V into a page that
        more than one table entry names (shared pages are read-only)."""
        P = self.page_size
        for s, p in zip(slots, positions):
            if p // P >= self._lead[s]:
                raise ValueError(
                    f"slot {s} position {p}: page {self._lead[s]} of the "
                    "slot is unmapped (set_slot_pages first)")
            page = self.table[s][p // P]
            if self.users[page] > 1:
                raise ValueError(
                    f"slot {s} position {p} would write into page {page}, "
                    f"which {self.users[page]} table entries share")


def is_decode_step(slots: list[int]) -> bool:
    """Every row belongs to another sequence: one decode row each."""
    return len(set(slots)) == len(slots)
