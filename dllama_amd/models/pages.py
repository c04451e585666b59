"""KV pages: a pool with reference counts and an index of shared prefixes.

A paged model keeps its KV cache as a pool of pages of `page_size` rows and
a page table per slot (docs/DESIGN.md §8). PagePool decides which pages a
sequence gets. It knows nothing of tensors: pages are ints 0..n_pages-1.

A page is in exactly one of three states:
  free     on the free list, holding nothing;
  in use   referenced by at least one running sequence;
  cached   referenced by nobody, but indexed: it holds the K/V of a known
           token prefix and can be matched again until it is evicted.

The prefix index is a trie over whole pages. A node is reached from the root
by the exact tokens of every page before it and of its own page, so a cached
page can only be matched by a prompt whose whole prefix, up to the end of
that page, equals the tokens the page was computed from. Evicting a node
drops its subtree from the index: a page below an evicted parent can never
become reachable through whatever is cached under the parent's key later.
"""

from __future__ import annotations

from collections import OrderedDict


class _Node:
    __slots__ = ("page", "parent", "key", "children")

    def __init__(self, page, parent, key):
        self.page = page
        self.parent = parent
        self.key = key            # this page's tokens, a tuple
        self.children = {}        # next page's tokens -> _Node


class PagePool:
    def __init__(self, n_pages: int, page_size: int, share: bool = True):
        if n_pages < 1:
            raise ValueError(f"n_pages must be >= 1 (got {n_pages})")
        if page_size < 1:
            raise ValueError(f"page_size must be >= 1 (got {page_size})")
        self.n_pages = n_pages
        self.page_size = page_size
        self.share = share        # False: match finds nothing, register no-op
        self.refs = [0] * n_pages
        self._free = list(range(n_pages - 1, -1, -1))  # pop() gives 0 first
        self._root = _Node(None, None, None)
        self._node = {}           # page -> its _Node while indexed
        # cached pages (indexed, zero references), least recently used first
        self._lru = OrderedDict()

    # ------------------------------------------------------------ counts

    @property
    def free(self) -> int:
        return len(self._free)

    @property
    def cached(self) -> int:
        return len(self._lru)

    @property
    def available(self) -> int:
        """Pages alloc could hand out now."""
        return len(self._free) + len(self._lru)

    def is_indexed(self, page: int) -> bool:
        return page in self._node

    # ------------------------------------------------------------ pages

    def alloc(self, n: int):
        """n pages with one reference each, or None (and no change) when
        free and evictable pages together are fewer than n. Free pages go
        first, then cached pages, least recently used first."""
        if n < 0:
            raise ValueError(f"alloc of {n} pages")
        if n > self.available:
            return None
        out = []
        for _ in range(n):
            if not self._free:
                self._evict(next(iter(self._lru)))
            page = self._free.pop()
            self.refs[page] = 1
            out.append(page)
        return out

    def _evict(self, page: int) -> None:
        """Drop a cached page and everything indexed below it. Unreferenced
        pages of the subtree become free; referenced ones stay with their
        sequences and are freed on release."""
        node = self._node[page]
        del node.parent.children[node.key]
        stack = [node]
        while stack:
            nd = stack.pop()
            stack.extend(nd.children.values())
            del self._node[nd.page]
            if self.refs[nd.page] == 0:
                del self._lru[nd.page]
                self._free.append(nd.page)

    def release(self, pages) -> None:
        """Drop one reference of every page. At zero an indexed page stays
        cached, an unindexed one is free again."""
        # last page first: the end of a chain is the older entry of the LRU
        # order, so a chain is evicted from its leaf
        for page in reversed(list(pages)):
            if self.refs[page] < 1:
                raise ValueError(f"page {page} released without a reference")
            self.refs[page] -= 1
            if self.refs[page] == 0:
                if page in self._node:
                    self._lru[page] = None
                else:
                    self._free.append(page)

    # ------------------------------------------------------------ prefixes

    def _keys(self, tokens, n_pages: int):
        P = self.page_size
        return [tuple(tokens[i * P: (i + 1) * P]) for i in range(n_pages)]

    def match(self, prompt) -> list[int]:
        """The longest run of cached full pages that spells the start of
        prompt, one reference taken on each. At most (len(prompt)-1) //
        page_size pages: at least one prompt token is left to feed, so the
        sequence's first step yields logits."""
        if not self.share:
            return []
        node, out = self._root, []
        for key in self._keys(prompt, (len(prompt) - 1) // self.page_size):
            node = node.children.get(key)
            if node is None:
                break
            out.append(node.page)
        for page in out:
            self.refs[page] += 1
            self._lru.pop(page, None)
        return out

    def register(self, prefix_tokens, page: int):
        """Index `page` as holding the last page_size positions of
        prefix_tokens (a whole number of pages, every position fed). Returns
        the page indexed under that prefix: `page`, the page that was there
        already (the existing entry is kept), or None when nothing was
        indexed (sharing off, or a page earlier in the chain is not cached
        any more)."""
        P = self.page_size
        if len(prefix_tokens) < P or len(prefix_tokens) % P:
            raise ValueError(
                f"a registered prefix is a whole number of pages of {P} "
                f"tokens (got {len(prefix_tokens)})")
        if not 0 <= page < self.n_pages or self.refs[page] < 1:
            raise ValueError(f"page {page} is not held by a sequence")
        if not self.share:
            return None
        keys = self._keys(prefix_tokens, len(prefix_tokens) // P)
        node = self._root
        for key in keys[:-1]:
            node = node.children.get(key)
            if node is None:
                return None
        have = node.children.get(keys[-1])
        if have is not None:
            return have.page
        if page in self._node:
            return None  # a page holds one prefix
        new = _Node(page, node, keys[-1])
        node.children[keys[-1]] = new
        self._node[page] = new
        return page
