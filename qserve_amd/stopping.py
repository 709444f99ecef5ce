"""Stop conditions on the device (extension; NOT part of the reference's `qserve_backend` surface - its stop checks are host Python):
stop sequences, per-sequence length limits and frozen rows for a decode loop that never reads its tokens back.

    stop_update   clip what one round (a decode step or a tree verification) is about to emit at the first stop, between the walk and
                  the commit: accept_lens / next_token / last_row are rewritten so that the commit, the advance of the lengths and the
                  history record handle the clipped path unchanged, and `finished` takes the reason.  include/qserve_amd.h
                  (`qs_stop_update`) has the rule, in exact integers.
    stop_table    a list of token ids and / or id sequences -> the padded (stop_seqs, stop_lens) pair of the rule.
    MAX_STOPS, MAX_STOP_LEN   rows of a stop table, tokens per row.
    LIVE, STOPPED, LENGTH, NO_PAGES   the values of `finished` (NO_PAGES: set by the page pool's reserve, qserve_amd.paging - never by
                  stop_update, which treats it like any other non-zero value: the row is frozen).

Backed by qserve_amd/csrc/stop_update.hip.  DecodeEngine.set_stopping puts it behind the engine's heads; DecodeEngine.generate is the
loop."""
import torch

from .backend._util import check, expect, guard, lib, ptr, stream
from .drafting import MAX_TREE, _history, _rows, _typed

MAX_STOPS = 32                  # rows of a stop table
MAX_STOP_LEN = 8                # tokens per row
LIVE, STOPPED, LENGTH = 0, 1, 2  # `finished`: live, a stop sequence, the length limit
NO_PAGES = 3                    # ... refused pages by the page pool (paging.PagePool.reserve)


def stop_table(stops, device=None, num_rows=None, width=None):
    """`stops`: token ids and / or sequences of token ids (a single stop token is a sequence of one) -> (stop_seqs int32 [S, W],
    stop_lens int32 [S]) with S = num_rows (None: max(len(stops), 1)) and W = width (None: the longest sequence); unused rows have length
    0 (off), unused columns hold -1.  At most MAX_STOPS sequences of 1 .. MAX_STOP_LEN non-negative ids each."""
    rows = []
    for s in stops:
        single = not hasattr(s, "__iter__") or (isinstance(s, torch.Tensor) and s.dim() == 0)       # (an int of any kind, a 0-d tensor)
        row = [int(s)] if single else [int(t) for t in s]
        if not 1 <= len(row) <= MAX_STOP_LEN or min(row) < 0 or max(row) >= 1 << 31:
            raise ValueError(f"stop_table: {row} - a stop sequence has 1 .. {MAX_STOP_LEN} token ids in 0 .. 2^31 - 1")
        rows.append(row)
    S = max(len(rows), 1) if num_rows is None else int(num_rows)
    W = max([len(r) for r in rows] + [1]) if width is None else int(width)
    if len(rows) > S or not 1 <= S <= MAX_STOPS:
        raise ValueError(f"stop_table: {len(rows)} stop sequences in {S} rows (at most {MAX_STOPS})")
    if not 1 <= W <= MAX_STOP_LEN or any(len(r) > W for r in rows):
        raise ValueError(f"stop_table: width={W} (the longest sequence .. {MAX_STOP_LEN})")
    seqs = torch.full((S, W), -1, dtype=torch.int32)
    lens = torch.zeros((S,), dtype=torch.int32)
    for i, row in enumerate(rows):
        seqs[i, :len(row)] = torch.tensor(row, dtype=torch.int32)
        lens[i] = len(row)
    return (seqs, lens) if device is None else (seqs.to(device), lens.to(device))


def stop_update(history, lengths, next_token, finished, stop_seqs=None, stop_lens=None, limit_lens=None, prompt_lens=None, node_tokens=None,
                accept_idx=None, accept_lens=None, last_row=None, out_lens=None, check_root=False):
    """Clip one round at the first stop.  history int32 [B, cap] (rows may be padded) and lengths int32 [B] from BEFORE the round advances
    them: the text.  The round emits e_1 .. e_m, m = accept_lens[b] (int32 [B]; None: 1): e_j = node_tokens[b, accept_idx[b, j]] for
    j < m (node_tokens int64 [B, n], accept_idx int32 [B, max_accept]; both None for a plain step), e_m = next_token[b] (int64 [B]);
    e_j lands at text position lengths[b] - 1 + j.  k = the first j at which the text reaches limit_lens[b] (int32 [B] or None) or a row
    of the stop table (stop_seqs int32 [S, W], stop_lens int32 [S], `stop_table`; None: no row) ends, all of it at positions >=
    prompt_lens[b] (int32 [B] or None: 0); j = 0, the current token, is looked at only with `check_root`.  No stop: k = m.
    In place: accept_lens = k (out_lens, int32 [B], where accept_lens is None: created if not given), next_token = e_k (k = 0: the
    frozen token history[b, lengths[b] - 1]), last_row[b] (int64 [B] or None) = b * n + accept_idx[b, k - 1] where the path was cut,
    finished[b] (int32 [B]) = STOPPED / LENGTH.  A sequence whose `finished` is set on entry emits nothing.  -> the tensor k was written to."""
    what = "stopping.stop_update"
    B, cap, stride = _history(history, what)
    dev = history.device
    _rows(lengths, torch.int32, (B,), "lengths", dev, what)
    _rows(next_token, torch.int64, (B,), "next_token", dev, what)
    _rows(finished, torch.int32, (B,), "finished", dev, what)
    S, W = 0, 1
    if (stop_seqs is None) != (stop_lens is None):
        raise RuntimeError(f"{what}: stop_seqs and stop_lens come together")
    if stop_seqs is not None:
        _typed(stop_seqs, torch.int32, "stop_seqs")
        if stop_seqs.dim() != 2 or not 0 <= stop_seqs.size(0) <= MAX_STOPS or not 1 <= stop_seqs.size(1) <= MAX_STOP_LEN or stop_seqs.device != dev:
            raise RuntimeError(f"{what}: stop_seqs must be [0 .. {MAX_STOPS}, 1 .. {MAX_STOP_LEN}] on {dev}, got {tuple(stop_seqs.shape)} on "
                               f"{stop_seqs.device}")
        S, W = stop_seqs.shape
        _rows(stop_lens, torch.int32, (S,), "stop_lens", dev, what)
    for t, name in ((limit_lens, "limit_lens"), (prompt_lens, "prompt_lens"), (accept_lens, "accept_lens"), (out_lens, "out_lens")):
        if t is not None:
            _rows(t, torch.int32, (B,), name, dev, what)
    if last_row is not None:
        _rows(last_row, torch.int64, (B,), "last_row", dev, what)
    if (node_tokens is None) != (accept_idx is None):
        raise RuntimeError(f"{what}: node_tokens and accept_idx come together (a verification's draft and its path)")
    n = max_accept = 1
    if node_tokens is not None:
        for t, dt, name in ((node_tokens, torch.int64, "node_tokens"), (accept_idx, torch.int32, "accept_idx")):
            _typed(t, dt, name)
            if t.dim() != 2 or t.size(0) != B or not 1 <= t.size(1) <= MAX_TREE or t.device != dev:
                raise RuntimeError(f"{what}: {name} must be [{B}, 1 .. {MAX_TREE}] on {dev}, got {tuple(t.shape)} on {t.device}")
        n, max_accept = node_tokens.size(1), accept_idx.size(1)
        if accept_lens is None:
            raise RuntimeError(f"{what}: a path (accept_idx) needs its accept_lens")
    if accept_lens is None and out_lens is None:
        out_lens = torch.empty((B,), dtype=torch.int32, device=dev)
    expect(history, torch.int32, "history", contiguous=False)
    for t, name in ((lengths, "lengths"), (next_token, "next_token"), (finished, "finished"), (stop_seqs, "stop_seqs"), (stop_lens, "stop_lens"),
                    (limit_lens, "limit_lens"), (prompt_lens, "prompt_lens"), (node_tokens, "node_tokens"), (accept_idx, "accept_idx"),
                    (accept_lens, "accept_lens"), (out_lens, "out_lens"), (last_row, "last_row")):
        if t is not None:
            expect(t, t.dtype, name)
    res = accept_lens if accept_lens is not None else out_lens
    if B == 0:                         # (an empty tensor has no address to hand over)
        return res
    if S == 0:                         # (an empty table has no address either)
        stop_seqs = stop_lens = None
    with guard(history):
        check(lib.qs_stop_update(ptr(history), stride, cap, ptr(lengths), ptr(prompt_lens), ptr(node_tokens), ptr(accept_idx), ptr(accept_lens),
                                 None if accept_lens is not None else ptr(out_lens), ptr(next_token), ptr(last_row), ptr(stop_seqs),
                                 ptr(stop_lens), ptr(limit_lens), ptr(finished), B, n, max_accept, S, W, 1 if check_root else 0, stream()),
              what)
    return res
