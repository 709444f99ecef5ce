"""The page pool of the paged KV cache on the device (extension; NOT part of the reference's `qserve_backend` surface - its block manager
is host Python): a free stack of page indices, common to the K and V pools of every layer, and the two launches that move pages
between it and the rows of the per-layer pointer tables - so a decode loop under a captured graph grows its rows, and gives finished
rows' pages to new texts, without the host reading a length.

    PagePool      the state (free stack, count, page_ids, owned, starved, error; with refcounts=True also refs, the holders of every
                  page) over existing tables and pools, with
                  reserve      grow every row to what a round of `extra` new tokens writes - all or nothing per row, first come in
                               row order; a refused row is marked `starved` (and `finished` = stopping.NO_PAGES);
                  release      push the masked rows' pages back and point their table entries at the sink (counted: give up their
                               holds, and the cache's `drop_ids`; a page is pushed when its last holder lets go);
                  hold         (counted) map pages that have a holder into further rows, and take the cache's holds;
                  fork         (counted) branch rows off running texts: share the whole pages, copy the partly filled one;
                  free_pages, snapshot, check.
    SINK          page N of every pool tensor: what a table entry names that names no owned page.

include/qserve_amd.h (`qs_pages_reserve`, `qs_pages_release`; `qs_pages_reserve_refs`, `qs_pages_hold`, `qs_pages_unhold`, `qs_pages_fork`) has the rules, in exact integers.  Backed by qserve_amd/csrc/page_pool.hip.
DecodeEngine(page_pool=N) puts a pool under the engine."""
import torch

from . import append as appendmod
from .backend._util import check, expect, guard, lib, ptr, stream
from .drafting import _rows, _typed

MAX_ROWS = 1024                 # rows of a batch: one workgroup scans them


class PagePool:
    """A pool of N pages per layer under `tables` (per layer int64 [B, 2, mb], on the device) and `pools` (per layer the (K, V) pair of
    uint8 [N + 1, page_bytes] tensors; page N is the sink).  Creating it gives every page to the free stack - the first page popped is
    page 0 - and points every table entry at the sink.  Every state tensor is persistent and filled in place: a captured reserve or
    release stays valid.

    `refcounts`: the pool also owns `refs` int32 [N], the holders of every page, and a scratch of 2 N words: `reserve` and `release` go
    through the counted entries (qs_pages_reserve_refs, qs_pages_unhold), and `hold` maps pages that already have a holder into further
    rows - what qserve_amd.prefix shares whole prompt pages with.  Without it the pool calls the two uncounted entries, as ever."""

    def __init__(self, tables, pools, page_bytes, refcounts=False):
        what = "paging.PagePool"
        tables, pools = tuple(tables), tuple(tuple(p) for p in pools)
        if not tables or len(tables) != len(pools):
            raise RuntimeError(f"{what}: one (K, V) pool pair per layer's table, got {len(tables)} tables and {len(pools)} pairs")
        self.layer_tables = appendmod.layer_table_pointers(tables)          # (checks the tables: int64 [B, 2, mb], one shape and device)
        dev = tables[0].device
        self.B, self.mb, self.L, self.page_bytes = tables[0].size(0), tables[0].size(2), len(tables), int(page_bytes)
        if self.page_bytes < 1:
            raise RuntimeError(f"{what}: page_bytes={self.page_bytes}")
        if not 1 <= self.B <= MAX_ROWS or self.mb < 1:
            raise RuntimeError(f"{what}: the tables are {tuple(tables[0].shape)}: 1 .. {MAX_ROWS} rows (one workgroup scans them) of at least "
                               "one page")
        rows = pools[0][0].size(0) if isinstance(pools[0][0], torch.Tensor) and pools[0][0].dim() == 2 else 0
        for li, pair in enumerate(pools):
            if len(pair) != 2:
                raise RuntimeError(f"{what}: pools[{li}] must be the (K, V) pair of layer {li}")
            for t, name in zip(pair, (f"pools[{li}][0]", f"pools[{li}][1]")):
                _typed(t, torch.uint8, name)
                if tuple(t.shape) != (rows, self.page_bytes) or rows < 2 or t.device != dev:
                    raise RuntimeError(f"{what}: {name} must be [N + 1, page_bytes] = [{rows}, {self.page_bytes}] (N >= 1, the last page is "
                                       f"the sink) on {dev}, got {tuple(t.shape)} on {t.device}")
                expect(t, torch.uint8, name)
        self.N = rows - 1
        self.tables, self.pools = tables, pools
        i32 = dict(dtype=torch.int32, device=dev)
        self.free = torch.arange(self.N - 1, -1, -1, **i32)
        self.count = torch.full((1,), self.N, **i32)
        self.page_ids = torch.full((self.B, self.mb), -1, **i32)
        self.owned = torch.zeros((self.B,), **i32)
        self.starved = torch.zeros((self.B,), **i32)
        self.error = torch.zeros((1,), **i32)
        self.refs = self._scratch = None
        if refcounts:
            self.refs, self._scratch = torch.zeros((self.N,), **i32), torch.zeros((2 * self.N,), **i32)
        self.layer_bases = torch.tensor([[k.data_ptr(), v.data_ptr()] for k, v in pools], dtype=torch.int64).to(dev)
        for t, (k, v) in zip(tables, pools):
            t[:, 0] = k.data_ptr() + self.N * self.page_bytes
            t[:, 1] = v.data_ptr() + self.N * self.page_bytes

    def _state(self):
        return (ptr(self.free), ptr(self.count), ptr(self.page_ids), ptr(self.owned), ptr(self.starved), ptr(self.error),
                ptr(self.layer_tables), ptr(self.layer_bases))

    def reserve(self, lengths, extra, extra_rows=None, finished=None):
        """Grow every row to the pages that hold slots 0 .. max(lengths[b], 1) - 2 + e_b, e_b = extra_rows[b] (int32 [B]) or `extra` -
        what a round of e_b new tokens behind a text of lengths[b] (int32 [B]) writes; a row whose finished[b] (int32 [B] or None) is
        set does not grow.  Rows are served in row order while the free pages last, all or nothing per row; a refused row gets
        starved[b] = 1 and, where it was live, finished[b] = stopping.NO_PAGES.  One launch, nothing read back."""
        what = "paging.PagePool.reserve"
        dev = self.free.device
        _rows(lengths, torch.int32, (self.B,), "lengths", dev, what)
        for t, name in ((extra_rows, "extra_rows"), (finished, "finished")):
            if t is not None:
                _rows(t, torch.int32, (self.B,), name, dev, what)
        extra = int(extra)
        if extra < 0:
            raise RuntimeError(f"{what}: extra={extra} (>= 0: the tokens the round is about to write)")
        for t, name in ((lengths, "lengths"), (extra_rows, "extra_rows"), (finished, "finished")):
            if t is not None:
                expect(t, torch.int32, name)
        with guard(self.free):
            if self.refs is None:
                check(lib.qs_pages_reserve(*self._state(), ptr(lengths), ptr(extra_rows), ptr(finished), self.B, self.mb, self.L, self.N,
                                           self.page_bytes, extra, stream()), what)
            else:
                check(lib.qs_pages_reserve_refs(*self._state(), ptr(self.refs), ptr(lengths), ptr(extra_rows), ptr(finished), self.B,
                                                self.mb, self.L, self.N, self.page_bytes, extra, stream()), what)

    def _ids(self, ids, name, what):
        """A host list of page ids -> (int32 tensor on the device or None, their number); the range is checked here."""
        ids = [int(i) for i in ids]
        if len(ids) > self.N or any(not 0 <= i < self.N for i in ids):
            raise RuntimeError(f"{what}: {name} {ids} - at most {self.N} page ids in 0 .. {self.N - 1}")
        return (torch.tensor(ids, dtype=torch.int32).to(self.free.device) if ids else None), len(ids)

    def release(self, rows_mask, drop_ids=()):
        """Give the pages of every row with rows_mask[b] != 0 (int32 or bool [B] on the device; a bool mask is converted first, which a
        capture should not contain) back to the free stack, in row order, then in logical page order; their table entries name the
        sink again, their `owned` and `starved` are 0.  One launch, nothing read back.

        A counted pool gives up HOLDS instead (qs_pages_unhold): one per page of a masked row, then one per entry of `drop_ids` (a host
        list: the holds the prefix cache drops); a page goes back to the stack when its last holder lets go, at the position of its
        first mention."""
        what = "paging.PagePool.release"
        dev = self.free.device
        if isinstance(rows_mask, torch.Tensor) and rows_mask.dtype == torch.bool:
            rows_mask = rows_mask.to(torch.int32)
        _rows(rows_mask, torch.int32, (self.B,), "rows_mask", dev, what)
        expect(rows_mask, torch.int32, "rows_mask")
        if self.refs is None:
            if len(drop_ids):
                raise RuntimeError(f"{what}: drop_ids are holds of a counted pool - PagePool(..., refcounts=True)")
            with guard(self.free):
                check(lib.qs_pages_release(*self._state(), ptr(rows_mask), self.B, self.mb, self.L, self.N, self.page_bytes, stream()), what)
            return
        drop, n = self._ids(drop_ids, "drop_ids", what)
        with guard(self.free):
            check(lib.qs_pages_unhold(*self._state(), ptr(self.refs), ptr(self._scratch), ptr(rows_mask), ptr(drop), n, self.B, self.mb,
                                      self.L, self.N, self.page_bytes, stream()), what)

    def hold(self, rows_pages, hold_ids=()):
        """Map pages that already have a holder into rows that own nothing: `rows_pages` is a dict row -> list of page ids, the row's
        logical pages 0, 1, ..; `hold_ids` (a host list) are the pages the prefix cache takes one more hold of, each at most once.
        Every named page's count rises by the number of times it is named.  One launch (qs_pages_hold) behind one upload; a free page,
        a row that owns pages, an id twice in `hold_ids` are broken invariants (`check`)."""
        what = "paging.PagePool.hold"
        if self.refs is None:
            raise RuntimeError(f"{what}: the pool keeps no reference counts - PagePool(..., refcounts=True)")
        take, src = torch.zeros((self.B,), dtype=torch.int32), torch.zeros((self.B, self.mb), dtype=torch.int32)
        for r, ids in dict(rows_pages).items():
            r, ids = int(r), [int(i) for i in ids]
            if not 0 <= r < self.B or len(ids) > self.mb or any(not 0 <= i < self.N for i in ids):
                raise RuntimeError(f"{what}: row {r} <- {ids} - rows are 0 .. {self.B - 1}, at most {self.mb} page ids in 0 .. {self.N - 1}")
            take[r] = len(ids)
            src[r, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
        held, n = self._ids(hold_ids, "hold_ids", what)
        dev = self.free.device
        take, src = take.to(dev), src.to(dev)
        with guard(self.free):
            check(lib.qs_pages_hold(*self._state(), ptr(self.refs), ptr(self._scratch), ptr(take), ptr(src), ptr(held), n, self.B, self.mb,
                                    self.L, self.N, self.page_bytes, stream()), what)

    def fork(self, src_rows, lengths, finished=None):
        """Branch rows off running texts: `src_rows` is int32 [B] on the device - src_rows[d] >= 0 makes row d a destination of that row,
        negative leaves it alone - or a host dict dst -> src, uploaded once; `lengths` (int32 [B]) are the texts' lengths.  A destination
        (which must own nothing, and whose source must be no destination) shares the source's whole pages below slot lengths - 1, where
        every writer of either text writes from now on, and gets a fresh page with a copy of the partly filled one; it is refused -
        `starved`, and `finished` = stopping.NO_PAGES where it was live - when that page cannot be had or the source itself was refused
        pages.  One call of qs_pages_fork (two launches), nothing read back."""
        what = "paging.PagePool.fork"
        if self.refs is None:
            raise RuntimeError(f"{what}: the pool keeps no reference counts - PagePool(..., refcounts=True)")
        dev = self.free.device
        if isinstance(src_rows, dict):
            rows = torch.full((self.B,), -1, dtype=torch.int32)
            for d, s in src_rows.items():
                d, s = int(d), int(s)
                if not 0 <= d < self.B or not 0 <= s < self.B or d == s:
                    raise RuntimeError(f"{what}: row {d} <- row {s} - rows are 0 .. {self.B - 1}, and no row is its own source")
                rows[d] = s
            src_rows = rows.to(dev)
        _rows(src_rows, torch.int32, (self.B,), "src_rows", dev, what)
        _rows(lengths, torch.int32, (self.B,), "lengths", dev, what)
        if finished is not None:
            _rows(finished, torch.int32, (self.B,), "finished", dev, what)
        for t, name in ((src_rows, "src_rows"), (lengths, "lengths"), (finished, "finished")):
            if t is not None:
                expect(t, torch.int32, name)
        with guard(self.free):
            check(lib.qs_pages_fork(*self._state(), ptr(self.refs), ptr(src_rows), ptr(lengths), ptr(finished), self.B, self.mb, self.L,
                                    self.N, self.page_bytes, stream()), what)

    def rows_mask(self, rows):
        """int32 [B] on the device with ones at the row indices `rows` - what `release` takes."""
        rows = [int(r) for r in rows]
        if any(not 0 <= r < self.B for r in rows):
            raise RuntimeError(f"paging.PagePool.rows_mask: rows {rows} - row indices are 0 .. {self.B - 1}")
        m = torch.zeros((self.B,), dtype=torch.int32)
        m[rows] = 1
        return m.to(self.free.device)

    def free_pages(self):
        """The number of free pages: one read-back."""
        return int(self.count.cpu())

    def snapshot(self):
        """Host copies of the state, for tests: free, count (an int), page_ids, owned, starved, error (an int) as numpy arrays, and
        `tables`: int64 [L, B, 2, mb]; a counted pool's `refs` too."""
        extra = {} if self.refs is None else dict(refs=self.refs.cpu().numpy())
        return dict(**extra, free=self.free.cpu().numpy(), count=int(self.count.cpu()), page_ids=self.page_ids.cpu().numpy(),
                    owned=self.owned.cpu().numpy(), starved=self.starved.cpu().numpy(), error=int(self.error.cpu()),
                    tables=torch.stack([t.cpu() for t in self.tables]).numpy())

    def check(self, starved=False):
        """Raise if a launch met a broken invariant (`error`: the state it met is unchanged, and no longer to be trusted) or, with
        `starved`, if a row was refused pages and nothing else would tell (an engine without the stop rule).  One read-back."""
        state = torch.cat((self.error, self.starved)).cpu()
        if int(state[0]):
            raise RuntimeError("paging.PagePool: a reserve or release met a broken invariant (count outside 0 .. N, owned outside 0 .. "
                               "max_blocks, a page id outside 0 .. N - 1, or more pages released than the pool has) and changed nothing" +
                               ("" if self.refs is None else
                                "; or, with reference counts: a popped page that has holders, a hold of a free page, into a row that owns "
                                "pages or of more than max_blocks pages, an id twice in hold_ids, more holds given up than a page has; a fork off a "
                                "row outside the batch, off itself or off a destination of the same launch, into a row that owns pages, or "
                                "off a row that names a free page"))
        if starved and bool(state[1:].any()):
            rows = torch.nonzero(state[1:]).view(-1).tolist()
            raise RuntimeError(f"paging.PagePool: rows {rows} were refused pages (the pool of {self.N} pages is exhausted): what they wrote "
                               "since went to the sink")
