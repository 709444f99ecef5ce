"""Log-probabilities on the device (extension; NOT part of the reference's `qserve_backend` surface - its sampler layer computes them
with torch ops): for every token a round emits its log-probability, its rank and a short top list, from the round's fp16 logit rows,
reproducible and capturable in a hipGraph.

    logprob_rows   the plain form: row r is scored for ids[r]
    logprob_path   the path form: the rows on the accepted path of a tree verification (or a decode step with a per-sequence 0 / 1
                   count), each scored for the token that follows it - the next node on the path, or the bonus token -, written at the
                   token's text position
    new_logs       the four output tensors, filled with what a column nobody wrote holds (NaN, 0, -1, NaN)
    MAX_TOP        entries of a top list

include/qserve_amd.h (`qs_logprob_rows`) has the contract: the values describe softmax(logits / T) - top-k and top-p do not enter -, all
sums are exact integer sums (bit-identical run to run and under graph replay), rank and ids are decided by integer keys alone, a tie
class of any size is cut by index.  Backed by qserve_amd/csrc/logprob_rows.hip.  DecodeEngine.set_logprobs puts it behind the engine's
heads."""
import torch

from .backend._util import check, expect, guard, lib, ptr, stream
from .drafting import MAX_TREE, _rows, _typed

MAX_TOP = 32                    # entries of a top list


def new_logs(batch, cols, top, device):
    """-> (lp float32 [batch, cols] = NaN, rank int32 [batch, cols] = 0, top_ids int32 [batch, cols, top] = -1, top_lp float32
    [batch, cols, top] = NaN): what a column no slot wrote holds."""
    return (torch.full((batch, cols), float("nan"), dtype=torch.float32, device=device),
            torch.zeros((batch, cols), dtype=torch.int32, device=device),
            torch.full((batch, cols, top), -1, dtype=torch.int32, device=device),
            torch.full((batch, cols, top), float("nan"), dtype=torch.float32, device=device))


def _logits(logits, what):
    """Type and shape of the logit rows (the device is looked at last, so that a wrong shape is reported before a wrong device)."""
    _typed(logits, torch.float16, "logits")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise RuntimeError(f"{what}: logits must be [rows, n] with a unit column stride, got {tuple(logits.shape)}, strides {logits.stride()}")
    rows, n = logits.shape
    if n < 8 or logits.stride(0) < n or logits.stride(0) % 8 != 0:
        raise RuntimeError(f"{what}: n={n} must be >= 8 and the row stride {logits.stride(0)} a multiple of 8 that is >= n")
    return rows, n


def _top(top, what):
    top = int(top)
    if not 0 <= top <= MAX_TOP:
        raise RuntimeError(f"{what}: top={top} (0 .. {MAX_TOP})")
    return top


def _temperature(v, batch, dev, what):
    """A scalar -> (scalar, None); a device tensor [batch] -> (1.0, tensor)."""
    if isinstance(v, torch.Tensor):
        _rows(v, torch.float32, (batch,), "temperature", dev, what)
        return 1.0, v
    return float(v), None


def _outputs(out, batch, cols, top, dev, what):
    """The (lp, rank, top_ids, top_lp) of a call, checked: lp / rank [batch, cols] and the lists [batch, cols, top], unit inner
    strides, ONE row stride (in columns) for all of them - views of wider logs are fine.  rank may be None; so may the lists at
    top == 0.  -> (lp, rank, top_ids, top_lp, row stride)."""
    if len(out) != 4:
        raise RuntimeError(f"{what}: out is (lp, rank, top_ids, top_lp)")
    lp, rank, ids, tlp = out
    if lp is None or (top > 0 and (ids is None or tlp is None)):
        raise RuntimeError(f"{what}: out needs lp, and with top={top} both top lists")
    stride = lp.stride(0) if isinstance(lp, torch.Tensor) and lp.dim() == 2 and batch > 1 else cols
    for t, dt, name in ((lp, torch.float32, "out lp"), (rank, torch.int32, "out rank")):
        if t is None:
            continue
        _typed(t, dt, name)
        if tuple(t.shape) != (batch, cols) or t.device != dev or (cols > 1 and t.stride(1) != 1) or \
                (batch > 1 and (t.stride(0) != stride or stride < cols)):
            raise RuntimeError(f"{what}: {name} must be [{batch}, {cols}] on {dev} with a unit column stride and the row stride of lp, got "
                               f"{tuple(t.shape)}, strides {t.stride()} on {t.device}")
    if top == 0:
        ids = tlp = None
    for t, dt, name in ((ids, torch.int32, "out top_ids"), (tlp, torch.float32, "out top_lp")):
        if t is None:
            continue
        _typed(t, dt, name)
        if tuple(t.shape) != (batch, cols, top) or t.device != dev or (top > 1 and t.stride(2) != 1) or (cols > 1 and t.stride(1) != top) or \
                (batch > 1 and t.stride(0) != stride * top):
            raise RuntimeError(f"{what}: {name} must be [{batch}, {cols}, {top}] on {dev}, rows of {top} entries at the row stride of lp, got "
                               f"{tuple(t.shape)}, strides {t.stride()} on {t.device}")
    return lp, rank, ids, tlp, stride


def _on_device(tensors):
    """`expect` on every argument, after the dtype and shape checks: what is left is the device and contiguity."""
    for t, name, contiguous in tensors:
        if t is not None:
            expect(t, t.dtype, name, contiguous=contiguous)


def logprob_rows(logits, ids, temperature=1.0, top=0, out=None):
    """Row r of `logits` (fp16 [rows, n], n >= 8, a unit column stride and a row stride that is a multiple of 8) scored for ids[r]
    (int64 [rows]) under softmax(logits / temperature); `temperature`: a scalar or a float32 [rows] device tensor, < 1e-5 counts as 1.
    -> (lp float32 [rows], rank int32 [rows], top_ids int32 [rows, top], top_lp float32 [rows, top]; the lists are None at top == 0):
    lp = log softmax at the id (NaN for an id outside [0, n)), rank = 1 + the ids in front of it in the order (logit descending, index
    ascending; 0 for an id out of range), the lists = the first `top` ids of that order with a logit other than -inf and their lp, the
    tail id -1 / lp -inf.  `out`: such a 4-tuple to write into (rank may be None)."""
    what = "logprobs.logprob_rows"
    rows, n = _logits(logits, what)
    dev = logits.device
    top = _top(top, what)
    _rows(ids, torch.int64, (rows,), "ids", dev, what)
    temperature, seq_t = _temperature(temperature, rows, dev, what)
    if out is None:
        res = new_logs(rows, 1, top, dev)
    else:
        if len(out) != 4:
            raise RuntimeError(f"{what}: out is (lp, rank, top_ids, top_lp)")
        res = tuple(None if t is None or not isinstance(t, torch.Tensor) else t.unsqueeze(1) for t in out)
    lp, rank, tids, tlp, stride = _outputs(res, rows, 1, top, dev, what)
    _on_device(((logits, "logits", False), (ids, "ids", True), (seq_t, "temperature", True), (lp, "out lp", False), (rank, "out rank", False),
                (tids, "out top_ids", False), (tlp, "out top_lp", False)))
    if rows > 0:
        with guard(logits):
            check(lib.qs_logprob_rows(ptr(logits), logits.stride(0), n, None, None, None, ptr(ids), None, rows, 1, 1, temperature, ptr(seq_t),
                                      top, ptr(lp), ptr(rank), ptr(tids), ptr(tlp), stride, 1, stream()), what)
    sq = lambda t: None if t is None else t.squeeze(1)   # noqa: E731
    return sq(lp), sq(rank), sq(tids), sq(tlp)


def logprob_path(logits, node_tokens, accept_idx, accept_lens, next_token, lengths=None, temperature=1.0, top=0, out=None, cols=None):
    """The path form.  logits fp16 [B * n, V]: row b * n + i is node i of sequence b.  The round emits e_1 .. e_m per sequence, m =
    accept_lens[b] (int32 [B]; None: 1): e_j = node_tokens[b, accept_idx[b, j]] for j < m (node_tokens int64 [B, n], accept_idx int32
    [B, max_accept]; both None for a plain step, n = 1), e_m = next_token[b] (int64 [B]) - the convention of stopping.stop_update and
    drafting.history_append.  e_j is scored on the row of node accept_idx[b, j - 1] and written at column lengths[b] - 1 + j (`lengths`
    int32 [B] from BEFORE the round advances it: the token's text position), or j - 1 without `lengths`.  Columns beyond the outputs are
    skipped; slots j > m write nothing.  `temperature`: a scalar or float32 [B].  `out`: (lp float32 [B, cols], rank int32 [B, cols] or
    None, top_ids int32 [B, cols, top], top_lp float32 [B, cols, top]) - views of wider logs with one common row stride are fine; None:
    `new_logs(B, cols, top)` with cols = max_accept unless given.  -> the 4-tuple written to (the lists None at top == 0)."""
    what = "logprobs.logprob_path"
    rows, V = _logits(logits, what)
    dev = logits.device
    top = _top(top, what)
    _typed(next_token, torch.int64, "next_token")
    if next_token.dim() != 1:
        raise RuntimeError(f"{what}: next_token must be [B], got {tuple(next_token.shape)}")
    B = next_token.size(0)
    _rows(next_token, torch.int64, (B,), "next_token", dev, what)
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
    if rows != B * n:
        raise RuntimeError(f"{what}: logits has {rows} rows, {B} sequences of {n} nodes have {B * n}")
    for t, name in ((accept_lens, "accept_lens"), (lengths, "lengths")):
        if t is not None:
            _rows(t, torch.int32, (B,), name, dev, what)
    temperature, seq_t = _temperature(temperature, B, dev, what)
    if out is None:
        out = new_logs(B, max_accept if cols is None else int(cols), top, dev)
    if not isinstance(out[0], torch.Tensor) or out[0].dim() != 2:
        raise RuntimeError(f"{what}: out lp must be a [B, cols] tensor")
    ncols = out[0].size(1)
    lp, rank, tids, tlp, stride = _outputs(out, B, ncols, top, dev, what)
    _on_device(((logits, "logits", False), (next_token, "next_token", True), (node_tokens, "node_tokens", True), (accept_idx, "accept_idx", True),
                (accept_lens, "accept_lens", True), (lengths, "lengths", True), (seq_t, "temperature", True), (lp, "out lp", False),
                (rank, "out rank", False), (tids, "out top_ids", False), (tlp, "out top_lp", False)))
    if B > 0 and ncols > 0:
        with guard(logits):
            check(lib.qs_logprob_rows(ptr(logits), logits.stride(0), V, ptr(node_tokens), ptr(accept_idx), ptr(accept_lens), ptr(next_token),
                                      ptr(lengths), B, n, max_accept, temperature, ptr(seq_t), top, ptr(lp), ptr(rank), ptr(tids), ptr(tlp),
                                      stride, ncols, stream()), what)
    return lp, rank, tids, tlp
