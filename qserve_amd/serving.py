"""What `DecodeEngine.serve` decides, on the host alone: no engine, no device tensor, no kernel binding - the engine's loop performs what
a `Scheduler` says and tells it what it read back.  The policy: first come first served with head-of-line blocking; a row that ended
for want of pages is preempted, back to the FRONT of the queue; the pool's pages are accounted from the read-backs."""
from collections import deque


class Scheduler:
    """`requests`: (prompt_tokens, max_new_tokens) in order of arrival, for `batch` rows of `max_len` slots.  `starved`: the `finished`
    code of a row that was refused pages (stopping.NO_PAGES).  `pool_pages`: the pool's N (None: static pages, `static_pages` of them,
    and no accounting); `advance`: the tokens a round writes at most (1, or the tree's nodes).  Refuses, before any state exists, a
    request that can never fit.  A request is dict(i, prompt, start, max_new, preempted_at); `slots[b]` is the request in row b.

    `prefix`: a `prefix.PrefixCache` (needs a pool) - place() then charges a request only the pages its prompt cannot map from the cache
    (`peek`: the scheduler never changes the cache), counts the cached pages no row holds as obtainable, and says how many of them
    must be evicted before the admit; a request also carries `hit_tokens`, the cached tokens of each of its placements.

    A request may also be (prompt_tokens, max_new_tokens, n), 1 <= n <= batch: n SAMPLES of one prompt.  `reqs` is then the flat list of
    samples (i: the sample's index in it; a sample of a request with n > 1 also has `req`, the request's index, and `k`, 0 .. n - 1).
    Sample 0, the leader, waits in the queue with its `copies`; the group is placed only when n rows are free - the queue blocks until
    then -, the leader is charged as a request is and every follower ONE page, since ceil((P + 1) / 64) - floor(P / 64) = 1 for every P;
    `copy_rows` says, per leader row of the last place(), the followers' rows (what admit(copy_rows=) takes).  From then on every
    sample is a request of its own: it ends by itself, and a preempted one resumes alone, its text as the prompt.  While siblings of
    the placement still run, a member that retires is not credited the floor(P / 64) pages they share; the last one is."""

    def __init__(self, requests, batch, max_len, starved, pool_pages=None, advance=1, static_pages=0, prefix=None):
        assert prefix is None or pool_pages is not None, "serve: a prefix cache shares the pages of a pool"
        reqs, self.groups = [], []                                          # groups: (request, its samples) in order of arrival
        for i, (p, m, *n) in enumerate(requests):
            p, m = [int(t) for t in (p.tolist() if hasattr(p, "tolist") else p)], int(m)
            assert len(n) <= 1, f"serve: request {i} - (prompt_tokens, max_new_tokens) or (prompt_tokens, max_new_tokens, n)"
            n = int(n[0]) if n else 1
            assert 1 <= n <= batch, f"serve: request {i} asks for n={n} samples - 1 .. batch = {batch}: a group is placed as a whole"
            assert len(p) >= 1 and m >= 1, f"serve: request {i} - a prompt of at least one token and max_new_tokens >= 1"
            assert len(p) + m <= max_len, f"serve: request {i} can never fit max_len: prompt {len(p)} + max_new_tokens {m} > {max_len}"
            assert pool_pages is None or (len(p) + m - 1 + advance + 63) // 64 <= pool_pages, \
                f"serve: request {i} can never fit the pool: prompt {len(p)} + max_new_tokens {m} need " \
                f"{(len(p) + m - 1 + advance + 63) // 64} pages, the pool has {pool_pages}"
            assert pool_pages is None or (len(p) + 1 + 63) // 64 + n - 1 <= pool_pages, \
                f"serve: request {i} can never fit the pool: its prompt of {len(p)} tokens and {n - 1} further samples need " \
                f"{(len(p) + 1 + 63) // 64 + n - 1} pages at once, the pool has {pool_pages}"
            members = [dict(i=len(reqs) + k, prompt=p, start=len(p), max_new=m, preempted_at=[]) for k in range(n)]
            if n > 1:
                assert pool_pages is not None, f"serve: request {i} asks for n={n} samples - they share the pages of a page pool"
                for k, q in enumerate(members):
                    q.update(req=i, k=k)
                members[0]["copies"] = members[1:]
            reqs += members
            self.groups.append(members)
        self.B, self.N, self.starved, self.reqs = batch, pool_pages, starved, reqs
        self.queue, self.slots, self.results = deque(g[0] for g in self.groups), [None] * batch, [None] * len(reqs)
        self.copy_rows, self.forks = {}, {}                              # place(): leader row -> follower rows; row -> its placement
        self.fin, self.lens = [0] * batch, [1] * batch                   # the last observation
        self.free, self.owned = pool_pages, [0] * batch                  # free pages (None without a pool), pages per row
        self.stats = dict(rounds=0, read_backs=0, admitted=0, preempted=0, peak_pages=static_pages if pool_pages is None else 0)
        if len(reqs) > len(self.groups):
            self.stats["forked"] = 0
        self.prefix = prefix
        if prefix is not None:
            self.stats.update(hit_tokens=0, evicted=0, inserted_pages=0)
            for q in reqs:
                q["hit_tokens"] = []

    def ended(self):
        """-> (the occupied rows that ended by the last observation, those of them that starved), ascending."""
        ended = [b for b in range(self.B) if self.slots[b] is not None and self.fin[b] != 0]
        return ended, [b for b in ended if self.fin[b] == self.starved]

    def retire(self, texts=(), cached=None):
        """Free the rows of ended(), giving their pages back.  A starved row's request is preempted: `texts` has its text row (one per
        starved row, in row order - reading them is one read-back) and the request returns to the front of the queue, in row order, with
        prompt := the text so far; `start` and `max_new` stay, so its length limit and penalty window do; `preempted_at` gains the
        generated tokens it held.  Any other row's request is done: results[i] = dict(length, reason).  -> those (row, i).
        `cached` (with a prefix cache): row -> how many of its pages the cache holds too - those stay where they are when the row lets
        go, so only the others count as free again."""
        ended, starved = self.ended()
        assert len(texts) == len(starved)
        for b, text in zip(starved, texts):
            self.slots[b]["prompt"] = [int(t) for t in text[:self.lens[b]]]
            self.slots[b]["preempted_at"].append(self.lens[b] - self.slots[b]["start"])
        self.queue.extendleft(self.slots[b] for b in reversed(starved))
        self.stats["preempted"] += len(starved)
        self.stats["read_backs"] += 1 if starved else 0
        done = [(b, self.slots[b]["i"]) for b in ended if b not in starved]
        for b, i in done:
            self.results[i] = dict(length=self.lens[b], reason=self.fin[b])
        for b in ended:
            self.slots[b] = None
            fork = self.forks.pop(b, None)                                  # (the placement this row's text was forked in, if any)
            shared = 0
            if fork is not None:
                fork["rows"] -= 1
                shared = fork["shared"] if fork["rows"] > 0 else 0         # siblings still hold them: not free yet
            if self.free is not None:
                self.free, self.owned[b] = self.free + max(self.owned[b] - max((cached or {}).get(b, 0), shared), 0), 0
        return done

    def place(self):
        """Waiting requests into free rows, rows ascending, in order of arrival, while the free pages cover the ceil((P + 1) / 64) of
        each; the first that they do not cover blocks the queue, whatever is behind it.  -> (rows, their requests): what to admit.

        With a prefix cache a request is charged ceil((P + 1) / 64) - len(peek(prompt, P - 1)) pages, against the free pages and the
        cached pages that can be evicted without touching what this call peeked.  -> (rows, their requests, (n, keep)): evict n
        cached pages first, sparing the ids `keep` - n is 0 while the free pages cover the charge."""
        rows, charged, keep = [], 0, []
        empty, self.copy_rows = [b for b in range(self.B) if self.slots[b] is None], {}
        while empty and self.queue:
            copies = self.queue[0].get("copies", [])
            if 1 + len(copies) > len(empty):                                # a group waits for all its rows, and the queue with it
                break
            P = len(self.queue[0]["prompt"])
            need = (P + 1 + 63) // 64 + len(copies)
            if self.prefix is not None:
                hits = self.prefix.peek(self.queue[0]["prompt"], P - 1)
                if charged + need - len(hits) > self.free + self.prefix.evictable(keep + hits):
                    break
                keep, charged = keep + hits, charged + need - len(hits)
                self.queue[0]["hit_tokens"].append(64 * len(hits))
                self.stats["hit_tokens"] += 64 * len(hits)
            elif self.free is not None:
                if need > self.free:
                    break
                self.free -= need
            b = empty.pop(0)
            self.slots[b] = self.queue.popleft()
            rows.append(b)
            if copies:
                del self.slots[b]["copies"]
                fork = dict(rows=1 + len(copies), shared=P // 64)
                self.copy_rows[b], empty = empty[:len(copies)], empty[len(copies):]
                for r, q in zip([b] + self.copy_rows[b], [self.slots[b]] + copies):
                    self.slots[r], self.forks[r] = q, fork
                self.stats["forked"] += len(copies)
                self.stats["admitted"] += len(copies)
        self.stats["admitted"] += len(rows)
        if self.prefix is None:
            return rows, [self.slots[b] for b in rows]
        evict = max(charged - self.free, 0)
        self.free, self.stats["evicted"] = self.free + evict - charged, self.stats["evicted"] + evict
        return rows, [self.slots[b] for b in rows], (evict, keep)

    def idle(self):
        """Nothing runs, so nothing waits (with every page free a request fits - checked on entry): the loop is over."""
        assert self.slots.count(None) < self.B or not self.queue, "serve: a waiting request does not fit the empty pool"
        return self.slots.count(None) == self.B

    def observe(self, rounds, finished, lengths, free=None, owned=None):
        """The one read-back behind a burst of `rounds` rounds: `finished` and `lengths` per row and, under a pool, its free count and
        the pages every row owns - which replace the scheduler's own estimate."""
        self.stats["rounds"] += rounds
        self.stats["read_backs"] += 1
        self.fin, self.lens = list(finished), list(lengths)
        if self.N is not None:
            self.free, self.owned = int(free), list(owned)
            self.stats["peak_pages"] = max(self.stats["peak_pages"], self.N - self.free)

    def output(self, texts):
        """`texts[i]`: the text row of request i (read once, one read-back) -> serve()'s return value."""
        self.stats["read_backs"] += 1
        more = (lambda q: dict(hit_tokens=q["hit_tokens"])) if self.prefix is not None else (lambda q: {})
        one = lambda q: dict(tokens=list(texts[q["i"]][q["start"]:self.results[q["i"]]["length"]]), reason=self.results[q["i"]]["reason"],   # noqa: E731
                             preempted_at=q["preempted_at"])
        # a request with n > 1: its samples, and sample 0's entries on top
        return [dict(one(g[0]), **more(g[0]), **(dict(samples=[one(q) for q in g]) if len(g) > 1 else {})) for g in self.groups], self.stats
