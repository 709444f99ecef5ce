"""Beam search on the device (extension; NOT part of the reference's `qserve_backend` surface): the W best continuations of every group of
W rows of the fixed batch, and the in-place move of the rows that got another parent - capturable in a hipGraph, nothing read back.

    select      per group of `width` rows: the `width` best (row, token) continuations by score = cum + log-probability, handed out to
                slots so that a row with a surviving child keeps its best child in its own slot -> parent, next_token, cum_out, moved,
                src_rows, and the candidate lists they were chosen from
    move_rows   row d of every given tensor becomes row parent[d], in place, in one launch
    rank        the final order of a group's hypotheses under a length penalty, on the host
    MAX_WIDTH   rows of a group
    MAX_MOVE    tensors of one move_rows launch

include/qserve_amd.h (`qs_beam_select`, `qs_rows_move`) has the contracts: the candidate lists are bit-identical to the top lists of
`qs_logprob_rows`, the choice is made on integer keys and single fp32 additions, and every source of a move is a row that stays -
parent[parent[d]] == parent[d] -, so (moved, src_rows) are what `paging.PagePool.release` followed by `paging.PagePool.fork` take.
Backed by qserve_amd/csrc/beam_select.hip.  DecodeEngine.set_beams puts them behind the engine's head."""
import ctypes

import torch

from .backend._util import check, expect, guard, lib, ptr, stream
from .drafting import _rows, _typed
from .logprobs import _logits

MAX_WIDTH = 32                  # rows of a group: one wave merges their lists
MAX_MOVE = 16                   # tensors of one move: their addresses travel in the kernel argument


def select(logits, cum, finished, tokens, width, out=None):
    """logits fp16 [B, n] (n >= 8, a unit column stride, a row stride that is a multiple of 8), as the head left them; cum float32 [B],
    the score of every row's text (-inf: a dead row); finished int32 [B] (non-zero: a frozen row, which competes with cum alone and
    keeps tokens[b]); tokens int64 [B]; `width` W in 1 .. 32 with B % W == 0: rows g * W .. g * W + W - 1 form group g.
    -> (parent int32 [B], next_token int64 [B], cum_out float32 [B], moved int32 [B], src_rows int32 [B], cand_ids int32 [B, W], cand_lp
    float32 [B, W]): slot d continues the text of row parent[d] with next_token[d] at score cum_out[d]; a slot left over keeps its row
    with score -inf; moved[d] = (parent[d] != d); src_rows[d] = parent[d] where moved, else -1.  `out`: such a 7-tuple to write into
    (moved and src_rows may be None); cum_out must not be `cum`.  Two launches, nothing read back."""
    what = "beams.select"
    B, n = _logits(logits, what)
    dev = logits.device
    width = int(width)
    if not 1 <= width <= MAX_WIDTH or B % width:
        raise RuntimeError(f"{what}: width={width} (1 .. {MAX_WIDTH}) must divide the {B} rows: rows g * width .. form group g")
    _rows(cum, torch.float32, (B,), "cum", dev, what)
    _rows(finished, torch.int32, (B,), "finished", dev, what)
    _rows(tokens, torch.int64, (B,), "tokens", dev, what)
    if out is None:
        i32 = dict(dtype=torch.int32, device=dev)
        out = (torch.empty((B,), **i32), torch.empty((B,), dtype=torch.int64, device=dev),
               torch.empty((B,), dtype=torch.float32, device=dev), torch.empty((B,), **i32), torch.empty((B,), **i32),
               torch.empty((B, width), **i32), torch.empty((B, width), dtype=torch.float32, device=dev))
    if len(out) != 7:
        raise RuntimeError(f"{what}: out is (parent, next_token, cum_out, moved, src_rows, cand_ids, cand_lp)")
    parent, next_token, cum_out, moved, src_rows, cand_ids, cand_lp = out
    spec = ((parent, torch.int32, (B,), "out parent"), (next_token, torch.int64, (B,), "out next_token"),
            (cum_out, torch.float32, (B,), "out cum_out"), (moved, torch.int32, (B,), "out moved"),
            (src_rows, torch.int32, (B,), "out src_rows"), (cand_ids, torch.int32, (B, width), "out cand_ids"),
            (cand_lp, torch.float32, (B, width), "out cand_lp"))
    for t, dt, shape, name in spec:
        if t is None and name in ("out moved", "out src_rows"):
            continue
        _rows(t, dt, shape, name, dev, what)
    if cum_out.data_ptr() == cum.data_ptr() and B > 0:
        raise RuntimeError(f"{what}: cum_out must not be cum (a group reads the scores of all its rows while it writes) - keep two buffers")
    expect(logits, torch.float16, "logits", contiguous=False)
    for t, name in ((cum, "cum"), (finished, "finished"), (tokens, "tokens"), *((t, name) for t, _, _, name in spec)):
        if t is not None:
            expect(t, t.dtype, name)
    if B > 0:
        with guard(logits):
            check(lib.qs_beam_select(ptr(logits), logits.stride(0), n, ptr(cum), ptr(finished), ptr(tokens), B, width, ptr(parent),
                                     ptr(next_token), ptr(cum_out), ptr(moved), ptr(src_rows), ptr(cand_ids), ptr(cand_lp), stream()), what)
    return parent, next_token, cum_out, moved, src_rows, cand_ids, cand_lp


def move_rows(parent, tensors, error):
    """For every tensor of `tensors` (at most 16; each [B, ...] on parent's device with contiguous rows: a row stride equal to the row's
    size) and every row d with p = parent[d] != d (int32 [B]): row d becomes row p, in place.  A p outside the batch, or one that is
    itself a destination, sets error[0] = 1 (int32 [1]) and that row is skipped - `select` never produces one.  One launch, nothing read
    back."""
    what = "beams.move_rows"
    _typed(parent, torch.int32, "parent")
    if parent.dim() != 1:
        raise RuntimeError(f"{what}: parent must be [B], got {tuple(parent.shape)}")
    B, dev = parent.size(0), parent.device
    _rows(error, torch.int32, (1,), "error", dev, what)
    tensors = list(tensors)
    if len(tensors) > MAX_MOVE:
        raise RuntimeError(f"{what}: {len(tensors)} tensors, one launch moves at most {MAX_MOVE}")
    bases, sizes = (ctypes.c_void_p * MAX_MOVE)(), (ctypes.c_int64 * MAX_MOVE)()
    for i, t in enumerate(tensors):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"tensors[{i}] must be a torch.Tensor")
        row = t[0].numel() * t.element_size() if t.dim() >= 1 and t.size(0) > 0 else 0
        if t.dim() < 1 or t.size(0) != B or t.device != dev or (B > 0 and (row < 1 or not t.is_contiguous())):
            raise RuntimeError(f"{what}: tensors[{i}] must be [{B}, ...] on {dev}, contiguous, with rows of at least one byte, got "
                               f"{tuple(t.shape)}, strides {t.stride()} on {t.device}")
        expect(t, t.dtype, f"tensors[{i}]")
        bases[i], sizes[i] = t.data_ptr(), row
    expect(parent, torch.int32, "parent")
    expect(error, torch.int32, "error")
    if B > 0 and tensors:
        with guard(parent):
            check(lib.qs_rows_move(ptr(parent), B, bases, sizes, len(tensors), ptr(error), stream()), what)


def rank(cum, gen_lens, length_penalty=1.0):
    """The final order of hypotheses: score = cum / max(len, 1) ** length_penalty in float64 on the host, descending, ties by row ->
    (order: the row indices best first, scores: the float64 score of every row).  `cum`, `gen_lens`: sequences of equal length."""
    cum, gen_lens = [float(c) for c in cum], [int(n) for n in gen_lens]
    if len(cum) != len(gen_lens):
        raise RuntimeError(f"beams.rank: {len(cum)} scores for {len(gen_lens)} lengths")
    scores = [c / float(max(n, 1)) ** float(length_penalty) for c, n in zip(cum, gen_lens)]
    return sorted(range(len(cum)), key=lambda i: (-scores[i], i)), scores
