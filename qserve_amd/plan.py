"""Which kernel would the W4A8 GEMM dispatcher pick for a problem?  (`qs_w4a8_gemm_plan`; runs without a GPU.)"""
import ctypes as C

from ._lib import check, lib

FAMILIES = {1: "splitk", 2: "pair", 3: "ring", 4: "tiled", 5: "wide"}


def gemm_plan(M, N, K, per_group=False):
    """-> dict(family=..., **geometry).  ring: m_tiles, units, token_blocks, k_slices; tiled: tile_tokens;
    splitk: m_tiles, waves, slices, xcd_map."""
    buf = (C.c_int * 5)()
    check(lib.qs_w4a8_gemm_plan(int(bool(per_group)), M, N, K, C.cast(buf, C.c_void_p)), "w4a8 gemm plan")
    fam = FAMILIES.get(buf[0], "none")
    if fam == "ring":
        return dict(family=fam, m_tiles=buf[1], units=buf[2], token_blocks=buf[3], k_slices=buf[4])
    if fam in ("tiled", "wide"):
        return dict(family=fam, tile_tokens=32 * buf[1])
    if fam == "splitk":
        return dict(family=fam, m_tiles=buf[1], waves=buf[2], slices=buf[3], xcd_map=bool(buf[4]))
    return dict(family=fam)


ATTN_FAMILIES = {1: "mfma_kv4", 2: "mfma_kv8", 3: "valu"}


def attention_plan(batch, num_heads, num_kv_heads, max_blocks, timestep, int4_kv_cache=True):
    """-> dict(family, kv_splits, waves): the decode attention dispatcher's choice (`qs_attention_plan`)."""
    buf = (C.c_int * 3)()
    check(lib.qs_attention_plan(batch, num_heads, num_kv_heads, max_blocks, timestep, int(bool(int4_kv_cache)),
                                C.cast(buf, C.c_void_p)), "attention plan")
    return dict(family=ATTN_FAMILIES.get(buf[0], "none"), kv_splits=buf[1], waves=buf[2])


def append_attention_plan(batch, max_seqlen_q, num_heads, num_kv_heads):
    """-> dict(tile_tokens, q_tiles, waves): the append attention launcher's geometry (`qs_append_attention_plan`).  One
    workgroup serves `tile_tokens` new tokens of one KV head with all its query heads; all zero for an empty launch."""
    buf = (C.c_int * 3)()
    check(lib.qs_append_attention_plan(batch, max_seqlen_q, num_heads, num_kv_heads, C.cast(buf, C.c_void_p)),
          "append attention plan")
    return dict(tile_tokens=buf[0], q_tiles=buf[1], waves=buf[2])


def append_attention_split_plan(batch, max_seqlen_q, max_past, num_heads, num_kv_heads, int4_kv_cache=True):
    """-> dict(tile_tokens, q_tiles, waves, splits, workspace_bytes): what `qs_append_attention_split` launches when it is asked
    to choose (`qs_append_attention_split_plan`).  The first three are `append_attention_plan`'s; `splits` page ranges per
    sequence (1 = the un-split launch, which takes no workspace); all zero for an empty launch."""
    buf = (C.c_int * 5)()
    check(lib.qs_append_attention_split_plan(batch, max_seqlen_q, max_past, num_heads, num_kv_heads, int(bool(int4_kv_cache)),
                                             C.cast(buf, C.c_void_p)), "append attention split plan")
    return dict(tile_tokens=buf[0], q_tiles=buf[1], waves=buf[2], splits=buf[3], workspace_bytes=buf[4] * 1024)


def append_shared_plan(batch, max_seqlen_q, num_groups, max_group_tokens, max_prefix, max_suffix_past, num_heads, num_kv_heads,
                       int4_kv_cache=True):
    """-> dict(tile_tokens, q_tiles, waves, suffix_splits, group_q_tiles, prefix_splits, rec_waves_suffix, rec_waves_prefix,
    workspace_bytes): what `qs_append_attention_shared` launches when it is asked to choose (`qs_append_shared_plan`).  The first
    three are `append_attention_plan`'s.  `prefix_splits` = 0: "do not share" - the split entry's launch over the whole past
    (`suffix_splits` and the workspace are then `append_attention_split_plan`'s for max_prefix + max_suffix_past).  All zero for an
    empty launch."""
    buf = (C.c_int * 8)()
    check(lib.qs_append_shared_plan(batch, max_seqlen_q, num_groups, max_group_tokens, max_prefix, max_suffix_past, num_heads,
                                    num_kv_heads, int(bool(int4_kv_cache)), C.cast(buf, C.c_void_p)), "append shared plan")
    return dict(tile_tokens=buf[0], q_tiles=buf[1], waves=buf[2], suffix_splits=buf[3], group_q_tiles=buf[4], prefix_splits=buf[5],
                rec_waves_suffix=buf[6] & 0xFF, rec_waves_prefix=buf[6] >> 8, workspace_bytes=buf[7] * 1024)
