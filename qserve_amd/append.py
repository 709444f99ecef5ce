"""Append attention (extension; NOT part of the reference's `qserve_backend` surface): n >= 1 new tokens per sequence against a
context that already sits in the quantised KV4 / KV8 pages - chunked prefill, prefix reuse, verification of drafted tokens.

Sequence b has `past_lens[b]` tokens in its pages and `cu_seqlens_q[b + 1] - cu_seqlens_q[b]` new rows in the packed fp16
`qkv` buffer [T, (H + 2 Hkv) * 128] (the layout the prefill writer takes; n = 0 is legal).  include/qserve_amd.h has the contract:

    append_rope_update_kv_cache   new token i: q, k rotated at position past + i in place; K / V quantised into that position's slot
    append_attention              row i attends to keys 0 .. past + i: < past de-quantised from the pages, >= past in fp16 from qkv
    append                        the two, in that order -> out fp16 [T, H, 128]

`max_past` / `num_splits` (append_attention, append): split-KV for long contexts at small batch.  With both None the call is the
un-split `qs_append_attention`; otherwise `qs_append_attention_split` cuts every sequence's past into page ranges that run as
workgroups of their own and merges their partial results - `num_splits` ranges when given, else what the planner
(`qserve_amd.plan.append_attention_split_plan`) picks for the upper-bound hint `max_past`.

Shared prefixes (prefix reuse): batch-adjacent sequences whose K / V tables name the SAME pages for a common leading context form a
group; `shared_prefix_groups` builds the three device arrays that describe the groups:

    append_attention_shared       append_attention's result with a group's common pages read ONCE for all its new rows (through the
                                  first member's table), each sequence's own pages and new tokens behind them, one merge
    append_shared                 the (unchanged) writer, then append_attention_shared

`past = 0` is the prefill pair (apply_bias_rope_update_kv_cache + flash_attn_varlen_func), `n = 1` is single_query_attention.

Tree-draft verification (several drafted candidates per position, verified in one pass): the n <= 64 new rows of a sequence are the
nodes of a tree in topological order, `tree_mask` int64 [T] holds one 64-bit word per row (bit j of node i's word: "node i sees new
token j of its own sequence"; `tree_masks_from_parents` builds ancestor-closed words):

    append_tree_rope_update_kv_cache   node i: q, k rotated at position past + depth (depth = popcount(word) - 1), K / V into slot past + i
    append_tree_attention              row i attends to every cached key < past and to the new keys its word names - nothing else
    append_tree                        the two, in that order
    commit_path                        after acceptance: slots past .. past + m - 1 receive the accepted path's K / V; the slots behind
                                       them keep the rejected nodes' stale bytes, which every reader masks by the sequence length

    accept_greedy                      the greedy walk over the verified tree on the device: path, its length, the last accepted row and
                                       the token to go on with - nothing is read back
    commit_path_layers                 commit_path for every layer in one launch (`layer_table_pointers` builds its table of tables)

Backed by qserve_amd/csrc/append_attention.hip, append_attention_split.hip, append_shared.hip, append_tree.hip, tree_accept.hip and the
offset-aware writers in attention.hip."""
import torch

from .backend._util import check, expect, guard, lib, ptr, stream


def _check_common(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, int4_kv, what):
    expect(qkv, torch.float16, "qkv")
    expect(cu_seqlens_q, torch.int32, "cu_seqlens_q")
    expect(past_lens, torch.int32, "past_lens")
    expect(kv_pointers, torch.int64, "kv_pointers")
    H, Hkv = int(num_heads), int(num_kv_heads)
    if H <= 0 or Hkv <= 0 or H % Hkv != 0:
        raise RuntimeError(f"{what}: bad head counts H={H} Hkv={Hkv}")
    if H // Hkv > 8:
        raise NotImplementedError(f"{what}: {H // Hkv} query heads per KV head (1..8 are provided, as for decode)")
    if qkv.dim() != 2 or qkv.size(1) != (H + 2 * Hkv) * 128:
        raise RuntimeError(f"{what}: qkv must be [tokens, (H + 2 Hkv) * 128] = [T, {(H + 2 * Hkv) * 128}], got {tuple(qkv.shape)}")
    batch = past_lens.numel()
    if cu_seqlens_q.dim() != 1 or past_lens.dim() != 1 or cu_seqlens_q.numel() != batch + 1:
        raise RuntimeError(f"{what}: cu_seqlens_q must be [batch + 1] and past_lens [batch]")
    if kv_pointers.dim() != 3 or kv_pointers.size(0) != batch or kv_pointers.size(1) != 2:
        raise RuntimeError(f"{what}: kv_pointers must be [batch, 2, max_blocks], got {tuple(kv_pointers.shape)}")
    if int(size_per_token) != Hkv * (64 if int4_kv else 128):
        raise RuntimeError(f"{what}: size_per_token={size_per_token}, expected {Hkv * (64 if int4_kv else 128)}")
    return batch


def append_rope_update_kv_cache(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, rope_theta,
                                int4_kv):
    """In place on `qkv` (q and k heads rotated at positions past + i) and on the pages behind `kv_pointers`."""
    what = "append.append_rope_update_kv_cache"
    batch = _check_common(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, int4_kv, what)
    with guard(qkv):
        check(lib.qs_append_rope_update_kv_cache(ptr(qkv), ptr(cu_seqlens_q), ptr(past_lens), ptr(kv_pointers), qkv.size(0), batch,
                                                 kv_pointers.size(-1), int(num_heads), int(num_kv_heads), 64, int(size_per_token),
                                                 128, float(rope_theta), int(bool(int4_kv)), 1, stream()), what)


def append_attention(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, int4_kv,
                     max_seqlen_q=None, out=None, max_past=None, num_splits=None):
    """`qkv` ALREADY rotated (append_rope_update_kv_cache) -> out fp16 [T, H, 128].  `max_seqlen_q`: an upper bound of the new
    tokens per sequence (sizes the launch; default: all T rows - correct, without a device read-back, but a larger grid).
    `max_past`: an upper bound of `past_lens` known on the host - a hint the split-KV planner sizes the launch with, never
    something the result depends on; `num_splits` >= 1 forces that many page ranges per sequence.  Both None: the un-split call."""
    what = "append.append_attention"
    batch = _check_common(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, int4_kv, what)
    T, H = qkv.size(0), int(num_heads)
    if out is None:
        out = torch.empty((T, H, 128), dtype=torch.float16, device=qkv.device)
    else:
        expect(out, torch.float16, "out", contiguous=False)
        if tuple(out.shape) != (T, H, 128) or out.stride(2) != 1 or out.stride(1) != 128 or out.stride(0) % 8 != 0:
            raise RuntimeError(f"{what}: out must be [T, H, 128] with contiguous heads and a row stride that is a multiple of 8")
    msq = T if max_seqlen_q is None else int(max_seqlen_q)
    if msq < 0:
        raise RuntimeError(f"{what}: max_seqlen_q={msq}")
    if num_splits is not None and int(num_splits) < 1:
        raise RuntimeError(f"{what}: num_splits={num_splits} (None, or a forced count >= 1)")
    args = (ptr(qkv), ptr(out), ptr(cu_seqlens_q), ptr(past_lens), ptr(kv_pointers), T, batch, min(msq, T), kv_pointers.size(-1), H,
            int(num_kv_heads), 128, qkv.stride(0), out.stride(0), 64, int(size_per_token), int(bool(int4_kv)), 1)
    with guard(qkv):
        if max_past is None and num_splits is None:
            check(lib.qs_append_attention(*args, stream()), what)
        else:
            hint = -1 if max_past is None else min(max(int(max_past), 0), 2 ** 31 - 1)
            check(lib.qs_append_attention_split(*args, hint, 0 if num_splits is None else int(num_splits), stream()), what)
    return out


def append(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, rope_theta, int4_kv,
           max_seqlen_q=None, max_past=None, num_splits=None):
    """Writer, then attention (the two touch disjoint page slots; the attention needs the writer's in-place rotation of qkv)."""
    append_rope_update_kv_cache(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, rope_theta,
                                int4_kv)
    return append_attention(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, int4_kv,
                            max_seqlen_q=max_seqlen_q, max_past=max_past, num_splits=num_splits)


# ---- shared prefixes ------------------------------------------------------------------------------------------------------------
def shared_prefix_groups(group_sizes, prefix_lens, device=None, batch=None):
    """Groups of batch-adjacent sequences with a common cached prefix -> (group_offsets int32 [groups + 1], prefix_lens int32 [groups],
    seq_group int32 [batch]) on `device` (built on the host).  Group g is the next `group_sizes[g]` sequences of the batch and shares
    `prefix_lens[g]` leading tokens - whole 64-token pages, 0 for "nothing shared".  Raises on an empty list, lists of different
    lengths, a size below 1, sizes that do not sum to `batch` (when given), and a prefix that is negative or no multiple of 64."""
    sizes = [int(x) for x in (group_sizes.tolist() if hasattr(group_sizes, "tolist") else group_sizes)]
    pref = [int(x) for x in (prefix_lens.tolist() if hasattr(prefix_lens, "tolist") else prefix_lens)]
    if not sizes or len(sizes) != len(pref):
        raise RuntimeError(f"shared_prefix_groups: {len(sizes)} group sizes and {len(pref)} prefix lengths (one each per group, at least one)")
    if any(n < 1 for n in sizes):
        raise RuntimeError(f"shared_prefix_groups: group sizes {sizes}: a group has at least one sequence")
    if batch is not None and sum(sizes) != int(batch):
        raise RuntimeError(f"shared_prefix_groups: group sizes {sizes} sum to {sum(sizes)}, not to the batch {batch}")
    if any(p < 0 or p % 64 for p in pref):
        raise RuntimeError(f"shared_prefix_groups: prefix lengths {pref}: a shared prefix is a non-negative multiple of 64 (whole pages)")
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + n)
    seq_group = [g for g, n in enumerate(sizes) for _ in range(n)]
    mk = lambda x: torch.tensor(x, dtype=torch.int32, device=device)      # noqa: E731
    return mk(offs), mk(pref), mk(seq_group)


def append_attention_shared(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, int4_kv, groups,
                            max_seqlen_q=None, out=None, max_group_tokens=None, max_prefix=None, max_suffix_past=None,
                            num_prefix_splits=None, num_suffix_splits=None):
    """`append_attention` (qkv ALREADY rotated -> out fp16 [T, H, 128]) for a batch in groups with common leading pages.  `groups`: the
    triple of `shared_prefix_groups`; the caller keeps the members' table entries below prefix / 64 equal to the first member's and
    every member's past >= its group's prefix.  `max_group_tokens`: an upper bound of a group's new tokens (default: all T rows);
    `max_prefix` / `max_suffix_past`: upper bounds of the prefixes / of past - prefix known on the host - planner hints, never
    something the result depends on.  `num_prefix_splits` / `num_suffix_splits`: None asks the planner, >= 1 forces the count,
    `num_prefix_splits=-1` forces "do not share" (the split-KV call over the whole past)."""
    what = "append.append_attention_shared"
    batch = _check_common(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, int4_kv, what)
    try:
        group_offsets, prefix_lens, seq_group = groups
    except (TypeError, ValueError):
        raise RuntimeError(f"{what}: groups must be the (group_offsets, prefix_lens, seq_group) triple of shared_prefix_groups") from None
    expect(group_offsets, torch.int32, "group_offsets")
    expect(prefix_lens, torch.int32, "prefix_lens")
    expect(seq_group, torch.int32, "seq_group")
    ngroups = prefix_lens.numel()
    if group_offsets.dim() != 1 or prefix_lens.dim() != 1 or seq_group.dim() != 1 or group_offsets.numel() != ngroups + 1 or \
            seq_group.numel() != batch or not (batch == 0 or 1 <= ngroups <= batch):
        raise RuntimeError(f"{what}: group_offsets must be [groups + 1], prefix_lens [groups] and seq_group [batch] with 1 <= groups <= batch, "
                           f"got {tuple(group_offsets.shape)}, {tuple(prefix_lens.shape)}, {tuple(seq_group.shape)} for batch {batch}")
    T, H = qkv.size(0), int(num_heads)
    if out is None:
        out = torch.empty((T, H, 128), dtype=torch.float16, device=qkv.device)
    else:
        expect(out, torch.float16, "out", contiguous=False)
        if tuple(out.shape) != (T, H, 128) or out.stride(2) != 1 or out.stride(1) != 128 or out.stride(0) % 8 != 0:
            raise RuntimeError(f"{what}: out must be [T, H, 128] with contiguous heads and a row stride that is a multiple of 8")
    msq = T if max_seqlen_q is None else int(max_seqlen_q)
    mgt = T if max_group_tokens is None else int(max_group_tokens)
    if msq < 0 or mgt < 0:
        raise RuntimeError(f"{what}: max_seqlen_q={msq}, max_group_tokens={mgt}")
    if num_prefix_splits is not None and (int(num_prefix_splits) < -1 or int(num_prefix_splits) == 0):
        raise RuntimeError(f"{what}: num_prefix_splits={num_prefix_splits} (None, a forced count >= 1, or -1 = do not share)")
    if num_suffix_splits is not None and int(num_suffix_splits) < 1:
        raise RuntimeError(f"{what}: num_suffix_splits={num_suffix_splits} (None, or a forced count >= 1)")
    hint = lambda v: -1 if v is None else min(max(int(v), 0), 2 ** 31 - 1)      # noqa: E731
    with guard(qkv):
        check(lib.qs_append_attention_shared(ptr(qkv), ptr(out), ptr(cu_seqlens_q), ptr(past_lens), ptr(kv_pointers), ptr(group_offsets),
                                             ptr(prefix_lens), ptr(seq_group), T, batch, ngroups, min(msq, T), min(mgt, T),
                                             kv_pointers.size(-1), H, int(num_kv_heads), 128, qkv.stride(0), out.stride(0), 64,
                                             int(size_per_token), int(bool(int4_kv)), 1, hint(max_prefix), hint(max_suffix_past),
                                             0 if num_prefix_splits is None else int(num_prefix_splits),
                                             0 if num_suffix_splits is None else int(num_suffix_splits), stream()), what)
    return out


def append_shared(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, rope_theta, int4_kv, groups,
                  max_seqlen_q=None, max_group_tokens=None, max_prefix=None, max_suffix_past=None, num_prefix_splits=None,
                  num_suffix_splits=None):
    """Writer, then shared-prefix attention.  The writer is append_rope_update_kv_cache: new token i goes to slot past + i >= prefix, a
    page the sequence owns - the shared pages are only read."""
    append_rope_update_kv_cache(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, rope_theta,
                                int4_kv)
    return append_attention_shared(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, int4_kv, groups,
                                   max_seqlen_q=max_seqlen_q, max_group_tokens=max_group_tokens, max_prefix=max_prefix,
                                   max_suffix_past=max_suffix_past, num_prefix_splits=num_prefix_splits,
                                   num_suffix_splits=num_suffix_splits)


# ---- tree-draft verification ------------------------------------------------------------------------------------------------
MAX_TREE = 64      # nodes per sequence: one 64-bit word per row


def tree_masks_from_parents(parents, cu_seqlens_q):
    """Ancestor masks of draft trees -> int64 [T] (CPU; the bit pattern of the library's uint64 words).  `parents[t]` is the parent
    of row t as an index INTO ITS OWN SEQUENCE, -1 for a node that hangs off the context; nodes are in topological order, so a
    parent's index is below its child's (anything else raises).  Word of node i = word of its parent | bit i: ancestor-closed, own
    bit set; a chain gives (2 << i) - 1."""
    par = [int(x) for x in (parents.tolist() if hasattr(parents, "tolist") else parents)]
    cu = [int(x) for x in (cu_seqlens_q.tolist() if hasattr(cu_seqlens_q, "tolist") else cu_seqlens_q)]
    if not cu or cu[0] != 0 or cu[-1] != len(par) or any(b < a for a, b in zip(cu, cu[1:])):
        raise RuntimeError(f"tree_masks_from_parents: cu_seqlens_q {cu} does not partition {len(par)} rows")
    words = []
    for s, e in zip(cu, cu[1:]):
        if e - s > MAX_TREE:
            raise RuntimeError(f"tree_masks_from_parents: {e - s} nodes in one sequence (at most {MAX_TREE})")
        for i in range(e - s):
            p = par[s + i]
            if p < -1 or p >= i:
                raise RuntimeError(f"tree_masks_from_parents: node {i} has parent {p}: a parent is -1 or an EARLIER node "
                                   "(topological order)")
            words.append((words[s + p] if p >= 0 else 0) | (1 << i))
    return torch.tensor([w - (1 << 64) if w >= (1 << 63) else w for w in words], dtype=torch.int64)


def _check_tree(tree_mask, qkv, max_seqlen_q, what):
    expect(tree_mask, torch.int64, "tree_mask")
    if tree_mask.dim() != 1 or tree_mask.numel() != qkv.size(0):
        raise RuntimeError(f"{what}: tree_mask must be int64 [T] = [{qkv.size(0)}], one word per row of qkv, got {tuple(tree_mask.shape)}")
    if max_seqlen_q is not None and int(max_seqlen_q) > MAX_TREE:
        raise RuntimeError(f"{what}: max_seqlen_q={max_seqlen_q}: a tree has at most {MAX_TREE} nodes per sequence")


def append_tree_rope_update_kv_cache(qkv, cu_seqlens_q, past_lens, kv_pointers, tree_mask, num_heads, num_kv_heads, size_per_token,
                                     rope_theta, int4_kv):
    """In place on `qkv` (q and k heads of node i rotated at position past + depth) and on the pages (slot past + i)."""
    what = "append.append_tree_rope_update_kv_cache"
    batch = _check_common(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, int4_kv, what)
    _check_tree(tree_mask, qkv, None, what)
    with guard(qkv):
        check(lib.qs_append_tree_rope_update_kv_cache(ptr(qkv), ptr(cu_seqlens_q), ptr(past_lens), ptr(kv_pointers), ptr(tree_mask),
                                                      qkv.size(0), batch, kv_pointers.size(-1), int(num_heads), int(num_kv_heads), 64,
                                                      int(size_per_token), 128, float(rope_theta), int(bool(int4_kv)), 1, stream()), what)


def append_tree_attention(qkv, cu_seqlens_q, past_lens, kv_pointers, tree_mask, num_heads, num_kv_heads, size_per_token, int4_kv,
                          max_seqlen_q=None, out=None, max_past=None, num_splits=None):
    """`qkv` ALREADY rotated (append_tree_rope_update_kv_cache) -> out fp16 [T, H, 128].  `max_seqlen_q` (<= 64; default: min(T, 64)),
    `max_past`, `num_splits` as for append_attention; with both None the launch is un-split."""
    what = "append.append_tree_attention"
    batch = _check_common(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, int4_kv, what)
    _check_tree(tree_mask, qkv, max_seqlen_q, what)
    T, H = qkv.size(0), int(num_heads)
    if out is None:
        out = torch.empty((T, H, 128), dtype=torch.float16, device=qkv.device)
    else:
        expect(out, torch.float16, "out", contiguous=False)
        if tuple(out.shape) != (T, H, 128) or out.stride(2) != 1 or out.stride(1) != 128 or out.stride(0) % 8 != 0:
            raise RuntimeError(f"{what}: out must be [T, H, 128] with contiguous heads and a row stride that is a multiple of 8")
    msq = min(T, MAX_TREE) if max_seqlen_q is None else int(max_seqlen_q)
    if msq < 0:
        raise RuntimeError(f"{what}: max_seqlen_q={msq}")
    if num_splits is not None and int(num_splits) < 1:
        raise RuntimeError(f"{what}: num_splits={num_splits} (None, or a forced count >= 1)")
    hint = -1 if max_past is None else min(max(int(max_past), 0), 2 ** 31 - 1)
    splits = (1 if max_past is None else 0) if num_splits is None else int(num_splits)
    with guard(qkv):
        check(lib.qs_append_tree_attention(ptr(qkv), ptr(out), ptr(cu_seqlens_q), ptr(past_lens), ptr(kv_pointers), ptr(tree_mask), T, batch,
                                           min(msq, T), kv_pointers.size(-1), H, int(num_kv_heads), 128, qkv.stride(0), out.stride(0), 64,
                                           int(size_per_token), int(bool(int4_kv)), 1, hint, splits, stream()), what)
    return out


def append_tree(qkv, cu_seqlens_q, past_lens, kv_pointers, tree_mask, num_heads, num_kv_heads, size_per_token, rope_theta, int4_kv,
                max_seqlen_q=None, max_past=None, num_splits=None):
    """Tree writer, then tree attention (the attention needs the writer's in-place rotation of qkv)."""
    if max_seqlen_q is not None and int(max_seqlen_q) > MAX_TREE:      # (before the writer touches anything)
        raise RuntimeError(f"append.append_tree: max_seqlen_q={max_seqlen_q}: a tree has at most {MAX_TREE} nodes per sequence")
    append_tree_rope_update_kv_cache(qkv, cu_seqlens_q, past_lens, kv_pointers, tree_mask, num_heads, num_kv_heads, size_per_token,
                                     rope_theta, int4_kv)
    return append_tree_attention(qkv, cu_seqlens_q, past_lens, kv_pointers, tree_mask, num_heads, num_kv_heads, size_per_token, int4_kv,
                                 max_seqlen_q=max_seqlen_q, max_past=max_past, num_splits=num_splits)


def commit_path(kv_pointers, past_lens, accept_idx, accept_lens, num_kv_heads, size_per_token, int4_kv):
    """In place on the pages: for k < accept_lens[b], slot past + k of sequence b receives the bytes of slot past + accept_idx[b, k]
    (K and V, every KV head; data, scale, zero).  accept_idx int32 [batch, max_accept <= 64], rows strictly increasing; accept_lens
    int32 [batch].  The slots behind the path keep the rejected nodes' bytes; the caller advances its lengths."""
    what = "append.commit_path"
    expect(kv_pointers, torch.int64, "kv_pointers")
    expect(past_lens, torch.int32, "past_lens")
    expect(accept_idx, torch.int32, "accept_idx")
    expect(accept_lens, torch.int32, "accept_lens")
    batch = past_lens.numel()
    if kv_pointers.dim() != 3 or kv_pointers.size(0) != batch or kv_pointers.size(1) != 2:
        raise RuntimeError(f"{what}: kv_pointers must be [batch, 2, max_blocks], got {tuple(kv_pointers.shape)}")
    if accept_idx.dim() != 2 or accept_idx.size(0) != batch or accept_lens.dim() != 1 or accept_lens.numel() != batch:
        raise RuntimeError(f"{what}: accept_idx must be [batch, max_accept] and accept_lens [batch]")
    if accept_idx.size(1) > MAX_TREE:
        raise RuntimeError(f"{what}: max_accept={accept_idx.size(1)}: a path has at most {MAX_TREE} nodes")
    Hkv = int(num_kv_heads)
    if Hkv <= 0 or int(size_per_token) != Hkv * (64 if int4_kv else 128):
        raise RuntimeError(f"{what}: size_per_token={size_per_token}, expected {Hkv * (64 if int4_kv else 128)}")
    with guard(kv_pointers):
        check(lib.qs_kv_cache_commit_path(ptr(kv_pointers), ptr(past_lens), ptr(accept_idx), ptr(accept_lens), batch, accept_idx.size(1),
                                          kv_pointers.size(-1), Hkv, 64, int(size_per_token), int(bool(int4_kv)), 1, stream()), what)


# ---- the tail of a verification on the device (csrc/tree_accept.hip) ---------------------------------------------------------------
def _expect_host(t, dtype, name):
    """The host-side part of `expect` (type, dtype): lets the shape checks below come before the device check."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != dtype:
        raise RuntimeError(f"expected scalar type {dtype} for {name} but found {t.dtype}")


def accept_greedy(tokens, argmax, parents, cu_seqlens_q, max_accept=None, out=None):
    """The greedy walk of tree verification, on the device.  `tokens` / `argmax` int64 [T]: the token every node carries and the
    model's arg-max at every node; `parents` int32 [T]: the parent of a node as an index INTO ITS OWN SEQUENCE, -1 = hangs off the
    context; `cu_seqlens_q` int32 [batch + 1] (a sequence's nodes beyond 64 are ignored).  Per sequence with n >= 1 nodes: node 0 is
    accepted; from the current node `cur` the walk goes to the LOWEST c > cur with parents[c] == cur and tokens[c] == argmax[cur], until
    there is none or the path holds `max_accept` nodes (1 .. 64; default: min(T, 64)).  Malformed parents cannot make it loop or read
    elsewhere: only c > cur is ever a candidate.
    -> (accept_idx int32 [batch, max_accept] - the path, 0 behind it -, accept_lens int32 [batch], last_row int64 [batch] - the global row
    of the last accepted node, -1 for an empty sequence -, next_token int64 [batch] - argmax[last_row]; the entry of an empty sequence is
    NOT written: 0 in a tensor allocated here).  `out`: the four tensors to write into (a captured graph's persistent buffers)."""
    what = "append.accept_greedy"
    for t, dt, name in ((tokens, torch.int64, "tokens"), (argmax, torch.int64, "argmax"), (parents, torch.int32, "parents"),
                        (cu_seqlens_q, torch.int32, "cu_seqlens_q")):
        _expect_host(t, dt, name)
    if tokens.dim() != 1 or argmax.dim() != 1 or parents.dim() != 1 or argmax.numel() != tokens.numel() or parents.numel() != tokens.numel():
        raise RuntimeError(f"{what}: tokens, argmax and parents must be [T], one entry per node, got {tuple(tokens.shape)}, "
                           f"{tuple(argmax.shape)}, {tuple(parents.shape)}")
    if cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 1:
        raise RuntimeError(f"{what}: cu_seqlens_q must be [batch + 1], got {tuple(cu_seqlens_q.shape)}")
    T, batch = tokens.numel(), cu_seqlens_q.numel() - 1
    ma = max(1, min(T, MAX_TREE)) if max_accept is None else int(max_accept)
    if not 1 <= ma <= MAX_TREE:
        raise RuntimeError(f"{what}: max_accept={ma}: a path has 1 .. {MAX_TREE} nodes")
    if out is not None:
        try:
            accept_idx, accept_lens, last_row, next_token = out
        except (TypeError, ValueError):
            raise RuntimeError(f"{what}: out must be the (accept_idx, accept_lens, last_row, next_token) quadruple") from None
        for t, dt, name in ((accept_idx, torch.int32, "accept_idx"), (accept_lens, torch.int32, "accept_lens"),
                            (last_row, torch.int64, "last_row"), (next_token, torch.int64, "next_token")):
            _expect_host(t, dt, name)
        if tuple(accept_idx.shape) != (batch, ma) or any(tuple(t.shape) != (batch,) for t in (accept_lens, last_row, next_token)):
            raise RuntimeError(f"{what}: out must be accept_idx [batch, max_accept] = [{batch}, {ma}] and accept_lens, last_row, next_token "
                               f"[{batch}], got {tuple(accept_idx.shape)}, {tuple(accept_lens.shape)}, {tuple(last_row.shape)}, "
                               f"{tuple(next_token.shape)}")
    for t, dt, name in ((tokens, torch.int64, "tokens"), (argmax, torch.int64, "argmax"), (parents, torch.int32, "parents"),
                        (cu_seqlens_q, torch.int32, "cu_seqlens_q")):
        expect(t, dt, name)
    if out is None:
        d = tokens.device
        accept_idx = torch.empty((batch, ma), dtype=torch.int32, device=d)
        accept_lens = torch.empty((batch,), dtype=torch.int32, device=d)
        last_row = torch.empty((batch,), dtype=torch.int64, device=d)
        next_token = torch.zeros((batch,), dtype=torch.int64, device=d)
    else:
        for t, dt, name in ((accept_idx, torch.int32, "accept_idx"), (accept_lens, torch.int32, "accept_lens"),
                            (last_row, torch.int64, "last_row"), (next_token, torch.int64, "next_token")):
            expect(t, dt, name)
    with guard(tokens):
        check(lib.qs_tree_accept_greedy(ptr(tokens), ptr(argmax), ptr(parents), ptr(cu_seqlens_q), T, batch, ma, ptr(accept_idx),
                                        ptr(accept_lens), ptr(last_row), ptr(next_token), stream()), what)
    return accept_idx, accept_lens, last_row, next_token


def layer_table_pointers(tables):
    """Per-layer pointer tables (each int64 [batch, 2, max_blocks], all of one shape, on one device) -> int64 [L] on that device: entry l
    is the device address of tables[l] - what commit_path_layers takes.  Built on the host, once per set of tables; the result keeps
    references to the tables, so the addresses stay valid as long as it lives."""
    what = "append.layer_table_pointers"
    tables = tuple(tables)
    if not tables:
        raise RuntimeError(f"{what}: at least one layer")
    for i, t in enumerate(tables):
        _expect_host(t, torch.int64, f"tables[{i}]")
        if t.dim() != 3 or t.size(1) != 2 or t.shape != tables[0].shape:
            raise RuntimeError(f"{what}: every table must be [batch, 2, max_blocks] of one shape, got {tuple(t.shape)} for layer {i}")
    for i, t in enumerate(tables):
        expect(t, torch.int64, f"tables[{i}]")
        if t.device != tables[0].device:
            raise RuntimeError(f"{what}: tables[{i}] is on {t.device}, tables[0] on {tables[0].device}")
    out = torch.tensor([t.data_ptr() for t in tables], dtype=torch.int64).to(tables[0].device)
    out._qs_tables = tables          # (keeps the pointed-to tensors alive)
    return out


def commit_path_layers(layer_tables, past_lens, accept_idx, accept_lens, max_blocks, num_kv_heads, size_per_token, int4_kv):
    """`commit_path` for every layer in ONE launch.  `layer_tables` int64 [L]: `layer_table_pointers` of the layers' kv_pointers
    [batch, 2, max_blocks]; `max_blocks`: their last dimension; past_lens, accept_idx and accept_lens as for commit_path, common to the
    layers.  The pages end byte-identical to L calls of commit_path."""
    what = "append.commit_path_layers"
    for t, dt, name in ((layer_tables, torch.int64, "layer_tables"), (past_lens, torch.int32, "past_lens"),
                        (accept_idx, torch.int32, "accept_idx"), (accept_lens, torch.int32, "accept_lens")):
        _expect_host(t, dt, name)
    if layer_tables.dim() != 1 or layer_tables.numel() < 1:
        raise RuntimeError(f"{what}: layer_tables must be int64 [layers] with at least one layer, got {tuple(layer_tables.shape)}")
    batch = past_lens.numel()
    if past_lens.dim() != 1 or accept_idx.dim() != 2 or accept_idx.size(0) != batch or accept_lens.dim() != 1 or accept_lens.numel() != batch:
        raise RuntimeError(f"{what}: past_lens must be [batch], accept_idx [batch, max_accept] and accept_lens [batch]")
    if accept_idx.size(1) > MAX_TREE:
        raise RuntimeError(f"{what}: max_accept={accept_idx.size(1)}: a path has at most {MAX_TREE} nodes")
    Hkv, mb = int(num_kv_heads), int(max_blocks)
    if mb <= 0:
        raise RuntimeError(f"{what}: max_blocks={mb}")
    if Hkv <= 0 or int(size_per_token) != Hkv * (64 if int4_kv else 128):
        raise RuntimeError(f"{what}: size_per_token={size_per_token}, expected {Hkv * (64 if int4_kv else 128)}")
    tabs = getattr(layer_tables, "_qs_tables", None)
    if tabs is not None and (tabs[0].size(0) != batch or tabs[0].size(-1) != mb):
        raise RuntimeError(f"{what}: the layers' tables are {tuple(tabs[0].shape)}, not [batch, 2, max_blocks] = [{batch}, 2, {mb}]")
    for t, dt, name in ((layer_tables, torch.int64, "layer_tables"), (past_lens, torch.int32, "past_lens"),
                        (accept_idx, torch.int32, "accept_idx"), (accept_lens, torch.int32, "accept_lens")):
        expect(t, dt, name)
    with guard(layer_tables):
        check(lib.qs_kv_cache_commit_path_layers(ptr(layer_tables), layer_tables.numel(), ptr(past_lens), ptr(accept_idx), ptr(accept_lens),
                                                 batch, accept_idx.size(1), mb, Hkv, 64, int(size_per_token), int(bool(int4_kv)), 1,
                                                 stream()), what)
