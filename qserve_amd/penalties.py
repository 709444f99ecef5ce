"""Repetition, presence and frequency penalties (extension; NOT part of the reference's `qserve_backend` surface - its sampler layer
is torch ops): the three knobs of the reference's SamplingParams applied to fp16 logit rows in place, on the device and capturable in
a hipGraph, from the token history the n-gram drafter already keeps.

    penalize_rows   edit the rows of one decode step (n_nodes = 1) or of one tree verification (the row of node i sees the history
                    plus the drafted tokens on the path to i) in front of `argmax_rows_` / `sampling.sample_rows`.
                    include/qserve_amd.h (`qs_penalize_rows`) has the rule, operation by operation: a numpy float32 restatement is
                    bit-equal.

Backed by qserve_amd/csrc/penalize_rows.hip.  DecodeEngine.set_penalties puts it in front of the engine's heads."""
import torch

from .backend._util import check, expect, guard, lib, ptr, stream
from .drafting import MAX_TREE, _history, _rows, _typed

MAX_CAP = 65535 - (MAX_TREE - 1)        # 16-bit counts: the history's cap plus the longest path must fit (the library refuses more)


def _seq_param(v, B, name, dev, what):
    """A scalar -> (float, None); a float32 device tensor [B] -> (neutral scalar, tensor)."""
    if isinstance(v, torch.Tensor):
        _rows(v, torch.float32, (B,), name, dev, what)
        return None, v
    return float(v), None


def penalize_rows(logits, history, lengths, prompt_lens=None, node_tokens=None, parents=None, repetition=1.0, frequency=0.0,
                  presence=0.0):
    """Penalise the fp16 rows logits [B * n, V] in place: row b * n + i from the tokens of history[b, :lengths[b]] (int32 [B, cap], rows
    may be padded; lengths int32 [B]) followed by node_tokens[b, j] (int64 [B, n]) of the nodes j != 0 on the path root -> i of the tree
    parents int32 [n] (parents[0] = -1; n <= 64).  Without node_tokens n = 1 and the context is the history alone.  For every token t
    of the context: x = x / repetition if x > 0 else x * repetition, then x -= frequency * c_gen(t) + presence * (c_gen(t) > 0), where
    c_gen counts the occurrences at positions >= prompt_lens[b] (int32 [B]; None: 0 - everything counts as generated).  `repetition`,
    `frequency`, `presence`: a scalar each, or a float32 device tensor [B] for per-sequence values; a scalar repetition must be > 0.
    Logits of tokens outside the context, and every row of a sequence with neutral values (1, 0, 0), are not written.  Rows need V >= 8,
    a unit column stride and a row stride that is a multiple of 8; cap <= 65 472.  -> logits."""
    what = "penalties.penalize_rows"
    _typed(logits, torch.float16, "logits")
    if logits.dim() != 2 or (logits.size(1) > 1 and logits.stride(1) != 1):
        raise RuntimeError(f"{what}: logits must be [rows, n] with a unit column stride, got {tuple(logits.shape)}, strides {logits.stride()}")
    rows, n = logits.shape
    row_stride = max(logits.stride(0), n) if rows <= 1 else logits.stride(0)
    if n < 8 or row_stride < n or row_stride % 8 != 0:
        raise RuntimeError(f"{what}: n={n} must be >= 8 and the row stride {row_stride} a multiple of 8 that is >= n")
    B, cap, stride = _history(history, what)
    dev = history.device
    if logits.device != dev:
        raise RuntimeError(f"{what}: logits must be on {dev}, got {logits.device}")
    _rows(lengths, torch.int32, (B,), "lengths", dev, what)
    if prompt_lens is not None:
        _rows(prompt_lens, torch.int32, (B,), "prompt_lens", dev, what)
    nodes = 1
    if node_tokens is not None:
        _typed(node_tokens, torch.int64, "node_tokens")
        if node_tokens.dim() != 2 or node_tokens.size(0) != B or not 1 <= node_tokens.size(1) <= MAX_TREE or node_tokens.device != dev:
            raise RuntimeError(f"{what}: node_tokens must be [{B}, 1 .. {MAX_TREE}] on {dev}, got {tuple(node_tokens.shape)} on "
                               f"{node_tokens.device}")
        nodes = node_tokens.size(1)
        if parents is None:
            raise RuntimeError(f"{what}: node_tokens needs the tree's parents")
    if parents is not None:
        _typed(parents, torch.int32, "parents")
        if node_tokens is None:
            nodes = parents.numel() if parents.dim() == 1 else 0
        if parents.dim() != 1 or parents.numel() != nodes or not 1 <= nodes <= MAX_TREE or parents.device != dev:
            raise RuntimeError(f"{what}: parents must be [n] with 1 <= n <= {MAX_TREE} (the columns of node_tokens) on {dev}, got "
                               f"{tuple(parents.shape)} on {parents.device}")
    if rows != B * nodes:
        raise RuntimeError(f"{what}: logits must have B * n = {B} * {nodes} rows, got {rows}")
    rep, seq_rep = _seq_param(repetition, B, "repetition", dev, what)
    freq, seq_freq = _seq_param(frequency, B, "frequency", dev, what)
    pres, seq_pres = _seq_param(presence, B, "presence", dev, what)
    if rep is not None and not rep > 0.0:
        raise RuntimeError(f"{what}: repetition={rep} must be > 0")
    expect(logits, torch.float16, "logits", contiguous=False)
    expect(history, torch.int32, "history", contiguous=False)
    for t, name in ((lengths, "lengths"), (prompt_lens, "prompt_lens"), (node_tokens, "node_tokens"), (parents, "parents"),
                    (seq_rep, "repetition"), (seq_freq, "frequency"), (seq_pres, "presence")):
        if t is not None:
            expect(t, t.dtype, name)
    if B == 0:                         # (an empty tensor has no address to hand over)
        return logits
    with guard(logits):
        check(lib.qs_penalize_rows(ptr(logits), row_stride, n, ptr(history), stride, cap, ptr(lengths), ptr(prompt_lens), ptr(node_tokens),
                                   ptr(parents), B, nodes, 1.0 if seq_rep is not None else rep, 0.0 if seq_freq is not None else freq,
                                   0.0 if seq_pres is not None else pres, ptr(seq_rep), ptr(seq_freq), ptr(seq_pres), stream()), what)
    return logits
