"""Which token chains live in which pages of the pool, on the host alone: no engine, no device tensor, no kernel binding - `DecodeEngine`
(prefix_cache=True) and `serving.Scheduler` ask a `PrefixCache` what a prompt can map instead of recomputing, and tell it what a row
computed.  Only WHOLE pages of 64 tokens are cached: a node is one page, keyed by (its parent node, its 64 tokens, a salt), so a chain of
nodes from the root is a token prefix of 64 * depth tokens and the pages that hold its K / V in every layer.

The cache owns no page.  It says which device holds to take (`insert` -> the ids that are new to it) and to drop (`evict`); the counted
pool (`paging.PagePool(refcounts=True)`) keeps a page alive while the cache or a row holds it.  What the cache counts itself is the ROWS
that hold a cached page: such a page is never evicted, and a page that no row holds is evictable once no cached child hangs below it."""
import heapq

PAGE = 64


class _Node:
    __slots__ = ("parent", "key", "page", "rows", "stamp", "children")

    def __init__(self, parent, key, page, stamp):
        self.parent, self.key, self.page, self.rows, self.stamp, self.children = parent, key, page, 0, stamp, {}


class PrefixCache:
    def __init__(self):
        self.root = _Node(None, None, -1, 0)
        self.by_page = {}                      # page id -> its node
        self.clock = 0

    def __len__(self):
        return len(self.by_page)

    @staticmethod
    def _keys(tokens, pages, salt):
        tokens = [int(t) for t in (tokens.tolist() if hasattr(tokens, "tolist") else tokens)][:PAGE * pages]
        return [(tuple(tokens[PAGE * i:PAGE * (i + 1)]), salt) for i in range(pages)]

    def _chain(self, tokens, limit, salt):
        """The nodes of the longest cached chain over tokens[:64 k], 64 k <= min(limit, len(tokens))."""
        node, chain = self.root, []
        for key in self._keys(tokens, max(min(int(limit), len(tokens)), 0) // PAGE, salt):
            node = node.children.get(key)
            if node is None:
                break
            chain.append(node)
        return chain

    def peek(self, tokens, limit, salt=0):
        """The page ids of the longest chain of cached pages that covers tokens[:64 k] with 64 k <= limit.  No side effect."""
        return [n.page for n in self._chain(tokens, limit, salt)]

    def match(self, tokens, limit, salt=0):
        """`peek`, and every page of the chain is held by one more row and stamped as used now.  The caller maps the ids into a row
        (PagePool.hold) and says `row_released` with them when the row lets go."""
        chain = self._chain(tokens, limit, salt)
        self.clock += 1
        for n in chain:
            n.rows, n.stamp = n.rows + 1, self.clock
        return [n.page for n in chain]

    def insert(self, tokens, ids, salt=0):
        """Enter the whole pages of `tokens` - page i under ids[i], the row's logical page i; pages beyond len(ids) are left out - as held
        by that row.  -> the ids that were not cached yet: the cache must take a device hold of each, and the row now holds them in the
        cache's count as well (`row_released` later).  A position that is already cached under the same id is the row's own match and
        is walked over; one that is cached under ANOTHER id is not entered, and neither is anything behind it in this row - the chain
        must stay a chain of the cached ids.  An id that is cached at another position ends the walk in the same way."""
        ids = [int(i) for i in ids]
        node, new = self.root, []
        self.clock += 1
        for key, page in zip(self._keys(tokens, min(len(tokens) // PAGE, len(ids)), salt), ids):
            child = node.children.get(key)
            if child is None:
                if page in self.by_page:
                    break
                child = _Node(node, key, page, self.clock)
                child.rows = 1
                node.children[key] = self.by_page[page] = child
                new.append(page)
            elif child.page != page:
                break
            child.stamp = self.clock
            node = child
        return new

    def row_released(self, ids):
        """One row holder less for each of these pages (ids the cache does not know are skipped: the row's private pages)."""
        for i in ids:
            n = self.by_page.get(int(i))
            if n is not None:
                assert n.rows >= 1, f"prefix.PrefixCache.row_released: page {n.page} has no row holder"
                n.rows -= 1

    def row_held(self, ids):
        """One row holder more for each of these pages that the cache knows (the others are skipped) - the inverse of `row_released`:
        what a row is told that maps another row's pages without a `match` (a fork).  -> the ids it counted."""
        held = []
        for i in ids:
            n = self.by_page.get(int(i))
            if n is not None:
                n.rows += 1
                held.append(n.page)
        return held

    def _blocked(self, keep):
        """The nodes that leaf-first eviction cannot reach: held by a row or named in `keep`, and every ancestor of such a node."""
        blocked = set()
        for n in self.by_page.values():
            if n.rows > 0 or n.page in keep:
                while n is not self.root and n.page not in blocked:
                    blocked.add(n.page)
                    n = n.parent
        return blocked

    def evictable(self, keep=()):
        """The pages `evict(n, keep)` can deliver: no row holds them or anything cached below them, and they are neither in `keep` nor
        above a page that is."""
        return len(self.by_page) - len(self._blocked(set(int(i) for i in keep)))

    def evict(self, n, keep=()):
        """Drop up to `n` pages, least recently used first among the nodes with no cached child and no row holder, skipping `keep`;
        evicting a leaf may expose its parent.  -> their ids: the cache's device holds to drop (PagePool.release(drop_ids=))."""
        keep = set(int(i) for i in keep)
        ok = lambda m: not m.children and m.rows == 0 and m.page not in keep       # noqa: E731
        heap = [(m.stamp, m.page) for m in self.by_page.values() if ok(m)]
        heapq.heapify(heap)
        out = []
        while heap and len(out) < n:
            _, page = heapq.heappop(heap)
            node = self.by_page.pop(page)
            del node.parent.children[node.key]
            out.append(page)
            if node.parent is not self.root and ok(node.parent):
                heapq.heappush(heap, (node.parent.stamp, node.parent.page))
        return out
