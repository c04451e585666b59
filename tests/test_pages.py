"""PagePool: reference-counted KV pages and the exact-content prefix index.
Pure Python: no model, no tensor."""

import pytest

from dllama_amd.models.pages import PagePool

P = 4


def _toks(*pages):
    """A token list of whole pages: page value v is [v, v+1, v+2, v+3]."""
    return [v + i for v in pages for i in range(P)]


def _balanced(pool):
    in_use = sum(1 for r in pool.refs if r > 0)
    assert pool.free + pool.cached + in_use == pool.n_pages
    assert pool.available == pool.free + pool.cached


def test_alloc_release_refcounts():
    pool = PagePool(6, P)
    a = pool.alloc(4)
    assert sorted(a) == [0, 1, 2, 3] and len(set(a)) == 4
    assert all(pool.refs[p] == 1 for p in a)
    assert pool.free == 2 and pool.cached == 0
    assert pool.alloc(0) == []
    pool.release(a[:2])
    assert pool.free == 4 and all(pool.refs[p] == 0 for p in a[:2])
    with pytest.raises(ValueError):
        pool.release(a[:1])  # no reference left to drop
    pool.release(a[2:])
    assert pool.free == 6
    _balanced(pool)


def test_alloc_fails_whole():
    pool = PagePool(4, P)
    held = pool.alloc(3)
    refs = list(pool.refs)
    assert pool.alloc(2) is None
    assert pool.refs == refs and pool.free == 1  # nothing was taken
    assert pool.alloc(1) is not None
    assert pool.alloc(1) is None
    pool.release(held)
    assert len(pool.alloc(3)) == 3


def test_match_whole_pages_and_one_token_left():
    pool = PagePool(8, P)
    pages = pool.alloc(3)
    toks = _toks(10, 20, 30)
    for i, page in enumerate(pages):
        assert pool.register(toks[: (i + 1) * P], page) == page
    pool.release(pages)
    assert pool.cached == 3 and pool.free == 5
    # 12 tokens = exactly three cached pages: the last stays to be fed
    got = pool.match(toks)
    assert got == pages[:2] and [pool.refs[p] for p in pages] == [1, 1, 0]
    pool.release(got)
    # one more token: all three
    got = pool.match(toks + [99])
    assert got == pages
    pool.release(got)
    # a partial third page matches two; a differing first page none
    assert pool.match(toks[:11]) == pages[:2]
    pool.release(pages[:2])
    assert pool.match([11] + toks[1:] + [99]) == []
    # a prompt that differs inside page 2 stops before it
    other = toks[:5] + [77] + toks[6:] + [99]
    assert pool.match(other) == pages[:1]
    pool.release(pages[:1])
    assert pool.match(toks[:P]) == [] and pool.match([]) == []
    _balanced(pool)


def test_share_off():
    pool = PagePool(4, P, share=False)
    pages = pool.alloc(2)
    toks = _toks(10, 20)
    assert pool.register(toks[:P], pages[0]) is None
    assert pool.match(toks + [1]) == []
    pool.release(pages)
    assert pool.free == 4 and pool.cached == 0


def test_register_keeps_existing_key():
    pool = PagePool(4, P)
    a, b = pool.alloc(2)
    toks = _toks(10)
    assert pool.register(toks, a) == a
    assert pool.register(toks, b) == a  # the entry that was there stays
    assert pool.is_indexed(a) and not pool.is_indexed(b)
    pool.release([a, b])
    assert pool.cached == 1 and pool.free == 3  # b went back to the free list
    with pytest.raises(ValueError):
        pool.register(toks[:3], a)  # not a whole page
    with pytest.raises(ValueError):
        pool.register(toks, b)      # b is held by nobody


def test_lru_eviction_only_at_zero_references():
    pool = PagePool(4, P)
    pages = pool.alloc(4)
    for v, page in zip((10, 20, 30, 40), pages):
        pool.register(_toks(v), page)  # four one-page chains
    # release 20 first, then 10: 20 is the least recently used
    pool.release([pages[1]])
    pool.release([pages[0]])
    assert pool.cached == 2 and pool.free == 0
    assert pool.alloc(3) is None  # 30 and 40 are referenced: never handed out
    got = pool.alloc(1)
    assert got == [pages[1]]      # evicted: least recently used
    assert pool.match(_toks(20) + [1]) == []
    # a match makes 10 recently used again: it outlives a later release
    hit = pool.match(_toks(10) + [1])
    assert hit == [pages[0]]
    pool.release([pages[2]])
    pool.release(hit)
    assert pool.alloc(1) == [pages[2]]
    assert pool.match(_toks(10) + [1]) == [pages[0]]
    assert pool.refs[pages[3]] == 1 and pool.is_indexed(pages[3])


def test_chain_evicts_leaf_first():
    pool = PagePool(3, P)
    pages = pool.alloc(3)
    toks = _toks(10, 20, 30)
    for i, page in enumerate(pages):
        pool.register(toks[: (i + 1) * P], page)
    pool.release(pages)
    assert pool.alloc(1) == [pages[2]]
    got = pool.match(toks + [1])
    assert got == pages[:2]  # the chain's head is still whole


def test_stale_parent_is_unreachable():
    """Chain A -> B. A is evicted while B is still held, A's page is reused
    for other tokens and registered; a prompt spelling the new A followed
    by the old B's tokens must not find the old B."""
    pool = PagePool(2, P)
    a, b = pool.alloc(2)
    old = _toks(10, 20)
    pool.register(old[:P], a)
    pool.register(old, b)
    pool.release([a])               # B's sequence still runs
    assert pool.alloc(1) == [a]     # A evicted, its page handed out again
    new_a = _toks(50)
    assert pool.register(new_a, a) == a
    pool.release([a])
    got = pool.match(new_a + old[P:] + [1])
    assert got == [a]               # new A only: old B hangs under no one
    pool.release(got)
    assert pool.match(old + [1]) == []
    assert not pool.is_indexed(b)
    pool.release([b])
    assert pool.free == 1 and pool.cached == 1
    _balanced(pool)


def test_register_below_evicted_parent_is_not_indexed():
    pool = PagePool(3, P)
    a, b = pool.alloc(2)
    toks = _toks(10, 20)
    pool.register(toks[:P], a)
    pool.release([a])
    c, = pool.alloc(1)
    assert pool.alloc(1) == [a]          # evicts A
    assert pool.register(toks, b) is None  # its parent is gone
    assert pool.match(toks + [1]) == []
    pool.release([a, b, c])
    assert pool.free == 3


def test_everything_comes_back():
    pool = PagePool(8, P)
    runs = []
    for v in (10, 10, 50):
        toks = _toks(v, v + 1000)
        shared = pool.match(toks + [1])
        pages = shared + pool.alloc(3 - len(shared))
        for i in range(len(shared), 2):
            pool.register(toks[: (i + 1) * P], pages[i])
        runs.append(pages)
        _balanced(pool)
    assert runs[1][:2] == runs[0][:2] and pool.refs[runs[0][0]] == 2
    for pages in runs:
        pool.release(pages)
        _balanced(pool)
    assert all(r == 0 for r in pool.refs)
    assert pool.free + pool.cached == pool.n_pages and pool.cached == 4
