"""N-gram (prompt-lookup) tree drafter (extension; NOT part of the reference's `qserve_backend` surface): the proposing half of
speculative decoding, on the device and capturable in a hipGraph - no second model, no weights.

    ngram_draft_tree   one draft tree per sequence from the sequence's own token history: every node continues the longest, then most
                       recent, earlier occurrence of its context that an earlier sibling has not used.  include/qserve_amd.h
                       (`qs_ngram_draft_tree`) has the rule, in exact integers.
    history_append     record what a verification accepted (the path's tokens, then the bonus token) behind the history.
    LDS_TOKENS         the history length up to which the drafter works from LDS; longer histories are read from global memory, with
                       the same results.

Backed by qserve_amd/csrc/ngram_draft.hip.  DecodeEngine.enable_drafting / draft_tree / speculate / capture_speculate close the loop."""
import torch

from .backend._util import check, expect, guard, lib, ptr, stream

MAX_TREE = 64                   # nodes per tree (qserve_amd.append.MAX_TREE)
MAX_NGRAM = 16                  # longest match looked for
# (None under QS_AMD_LIBRARY_AB=1 with an older build that lacks the drafter: importing this module must not fail there)
LDS_TOKENS = int(lib.qs_ngram_draft_lds_tokens()) if hasattr(lib, "qs_ngram_draft_lds_tokens") else None


def _typed(t, dtype, name):
    """The type and dtype half of `expect`, so that a wrong shape is reported before a wrong device."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != dtype:
        raise RuntimeError(f"expected scalar type {dtype} for {name} but found {t.dtype}")


def _history(history, what):
    _typed(history, torch.int32, "history")
    if history.dim() != 2 or history.size(1) < 1 or (history.size(0) > 1 and history.stride(0) < history.size(1)) or \
            (history.size(1) > 1 and history.stride(1) != 1):
        raise RuntimeError(f"{what}: history must be [B, cap] (cap >= 1) with a unit column stride and a row stride >= cap, got "
                           f"{tuple(history.shape)}, strides {history.stride()}")
    return history.size(0), history.size(1), max(history.stride(0), history.size(1))


def _rows(t, dtype, shape, name, dev, what):
    _typed(t, dtype, name)
    if tuple(t.shape) != shape or t.device != dev:
        raise RuntimeError(f"{what}: {name} must be {list(shape)} on {dev}, got {tuple(t.shape)} on {t.device}")


def _on_device(history, rest):
    """`expect` on every argument, after the dtype and shape checks: what is left is the device and contiguity."""
    expect(history, torch.int32, "history", contiguous=False)
    for t, name in rest:
        expect(t, t.dtype, name)


def ngram_draft_tree(history, lengths, parents, max_ngram=4, min_match=1, pad_token=0, out=None):
    """out[b, i] = the drafted token of node i of sequence b (int64 [B, n]) from history int32 [B, cap] (rows may be padded: a row stride
    >= cap), lengths int32 [B] and the tree parents int32 [n] on the device (parents[0] = -1, 0 <= parents[i] < i; n <= 64).  Column 0
    is history[b, lengths[b] - 1], the root.  1 <= min_match <= max_ngram <= 16.  -> out."""
    what = "drafting.ngram_draft_tree"
    B, cap, stride = _history(history, what)
    dev = history.device
    _rows(lengths, torch.int32, (B,), "lengths", dev, what)
    _typed(parents, torch.int32, "parents")
    if parents.dim() != 1 or not 1 <= parents.numel() <= MAX_TREE or parents.device != dev:
        raise RuntimeError(f"{what}: parents must be [n] with 1 <= n <= {MAX_TREE} on {dev}, got {tuple(parents.shape)} on {parents.device}")
    n = parents.numel()
    max_ngram, min_match = int(max_ngram), int(min_match)
    if not 1 <= min_match <= max_ngram <= MAX_NGRAM:
        raise RuntimeError(f"{what}: max_ngram={max_ngram}, min_match={min_match} (1 <= min_match <= max_ngram <= {MAX_NGRAM})")
    if out is None:
        out = torch.empty((B, n), dtype=torch.int64, device=dev)
    _rows(out, torch.int64, (B, n), "out", dev, what)
    _on_device(history, ((lengths, "lengths"), (parents, "parents"), (out, "out")))
    if B == 0:                         # (an empty tensor has no address to hand over)
        return out
    with guard(history):
        check(lib.qs_ngram_draft_tree(ptr(history), stride, cap, ptr(lengths), ptr(parents), B, n, max_ngram, min_match, int(pad_token),
                                      ptr(out), stream()), what)
    return out


def history_append(history, past_lens, node_tokens, accept_idx, accept_lens, next_token):
    """After a verification: history[b, past + j] = node_tokens[b, accept_idx[b, j]] for 1 <= j < m = accept_lens[b], and
    history[b, past + m] = next_token[b]; past_lens int32 [B] = lengths - 1 from before the verification advanced them, node_tokens
    int64 [B, n] (the draft), accept_idx int32 [B, max_accept], accept_lens int32 [B], next_token int64 [B].  Writes beyond the row's
    cap are skipped; nothing else changes.  -> history."""
    what = "drafting.history_append"
    B, cap, stride = _history(history, what)
    dev = history.device
    _rows(past_lens, torch.int32, (B,), "past_lens", dev, what)
    for t, dt, name in ((node_tokens, torch.int64, "node_tokens"), (accept_idx, torch.int32, "accept_idx")):
        _typed(t, dt, name)
        if t.dim() != 2 or t.size(0) != B or not 1 <= t.size(1) <= MAX_TREE or t.device != dev:
            raise RuntimeError(f"{what}: {name} must be [{B}, 1 .. {MAX_TREE}] on {dev}, got {tuple(t.shape)} on {t.device}")
    _rows(accept_lens, torch.int32, (B,), "accept_lens", dev, what)
    _rows(next_token, torch.int64, (B,), "next_token", dev, what)
    _on_device(history, ((past_lens, "past_lens"), (node_tokens, "node_tokens"), (accept_idx, "accept_idx"), (accept_lens, "accept_lens"),
                         (next_token, "next_token")))
    if B == 0:
        return history
    with guard(history):
        check(lib.qs_history_append(ptr(history), stride, cap, ptr(past_lens), ptr(node_tokens), ptr(accept_idx), ptr(accept_lens),
                                    ptr(next_token), B, node_tokens.size(1), accept_idx.size(1), stream()), what)
    return history
