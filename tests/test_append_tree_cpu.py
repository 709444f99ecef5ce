"""Tree-draft verification without a GPU: the mask builder on hand-written trees, the refusals of the Python wrappers and of the
three C entries (argument validation happens before any device call, on made-up addresses), and the pin of the float64 tree oracle
(tests/_tree_cases.py) to the existing composition for chains."""
import numpy as np
import pytest
import torch

from _append_cases import expected, rotate_rows, scattered_tables
from _tree_cases import chain_words, expected_tree, rotate_rows_tree, words_from_parents
from oracle import kvattn

BASE = 1e4
U64 = (1 << 64) - 1


def _words(t):
    return [int(x) & U64 for x in t.tolist()]


def test_tree_masks_from_parents_on_hand_written_trees(built_lib):
    from qserve_amd.append import tree_masks_from_parents as tm
    # a chain: (2 << i) - 1
    assert _words(tm([-1, 0, 1, 2, 3], [0, 5])) == [1, 3, 7, 15, 31]
    # a star: every leaf sees the root and itself
    assert _words(tm([-1, 0, 0, 0], [0, 4])) == [0b1, 0b11, 0b101, 0b1001]
    # two roots (the second hangs off the context too), one child each; then a second sequence whose indices start again at 0
    assert _words(tm([-1, -1, 0, 1, -1, 0], [0, 4, 6])) == [0b1, 0b10, 0b101, 0b1010, 0b1, 0b11]
    # an empty sequence between two others
    assert _words(tm([-1, -1, 0], [0, 1, 1, 3])) == [1, 1, 3]
    # n = 64: the chain's last word is all ones (the sign bit of the int64 the tensor holds), a comb's leaves see root + themselves
    chain = tm([-1] + list(range(63)), [0, 64])
    assert chain.dtype == torch.int64 and _words(chain) == chain_words(64) and int(chain[63]) == -1
    comb = tm([-1] + [0] * 63, [0, 64])
    assert _words(comb) == [1] + [1 | (1 << i) for i in range(1, 64)] and int(comb[63]) < 0
    # tensors are taken as well as lists
    assert _words(tm(torch.tensor([-1, 0, 0]), torch.tensor([0, 3], dtype=torch.int32))) == [1, 3, 5]
    assert _words(tm([-1, 0, 1, 1, 0, 4, -1], [0, 7])) == words_from_parents([-1, 0, 1, 1, 0, 4, -1])


def test_tree_masks_from_parents_refuses(built_lib):
    from qserve_amd.append import tree_masks_from_parents as tm
    with pytest.raises(RuntimeError, match="parent"):
        tm([-1, 1], [0, 2])                      # its own parent
    with pytest.raises(RuntimeError, match="parent"):
        tm([-1, 2, 0], [0, 3])                   # a later node
    with pytest.raises(RuntimeError, match="parent"):
        tm([-1, 0, -1, 1], [0, 2, 4])            # node 1 of the SECOND sequence: an index into the first
    with pytest.raises(RuntimeError, match="parent"):
        tm([-2], [0, 1])
    with pytest.raises(RuntimeError, match="at most 64"):
        tm([-1] * 65, [0, 65])
    with pytest.raises(RuntimeError, match="partition"):
        tm([-1, 0], [0, 3])


def test_python_wrappers_raise_before_the_library_is_touched(built_lib):
    from qserve_amd import append as A
    H, Hkv = 8, 2
    qkv = torch.zeros((4, (H + 2 * Hkv) * 128), dtype=torch.float16)     # CPU tensors: every call must fail in the checks
    cu = torch.tensor([0, 4], dtype=torch.int32)
    past = torch.zeros((1,), dtype=torch.int32)
    kvp = torch.zeros((1, 2, 2), dtype=torch.int64)
    mask = A.tree_masks_from_parents([-1, 0, 0, 1], cu)
    with pytest.raises(RuntimeError, match="max_seqlen_q=65"):
        A.append_tree(qkv, cu, past, kvp, mask, H, Hkv, Hkv * 64, BASE, True, max_seqlen_q=65)
    with pytest.raises(RuntimeError, match="CUDA"):
        A.append_tree(qkv, cu, past, kvp, mask, H, Hkv, Hkv * 64, BASE, True)
    with pytest.raises(RuntimeError, match="CUDA"):
        A.append_tree_attention(qkv, cu, past, kvp, mask, H, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="scalar type"):
        A.append_tree_rope_update_kv_cache(qkv.float(), cu, past, kvp, mask, H, Hkv, Hkv * 64, BASE, True)
    with pytest.raises(RuntimeError, match="CUDA"):
        A.commit_path(kvp, past, torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1,), dtype=torch.int32), Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="scalar type"):
        A.commit_path(kvp.to(torch.int32), past, torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1,), dtype=torch.int32), Hkv, Hkv * 64, True)


@pytest.mark.gpu
def test_python_wrappers_check_shapes(gpu):
    """(device tensors: the shape checks sit behind the device check; still no launch)"""
    from qserve_amd import append as A
    H, Hkv, d = 8, 2, gpu
    qkv = torch.zeros((4, (H + 2 * Hkv) * 128), dtype=torch.float16, device=d)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=d)
    past = torch.zeros((1,), dtype=torch.int32, device=d)
    kvp = torch.zeros((1, 2, 2), dtype=torch.int64, device=d)
    mask = torch.zeros((4,), dtype=torch.int64, device=d)
    with pytest.raises(RuntimeError, match="scalar type"):
        A.append_tree_attention(qkv, cu, past, kvp, mask.to(torch.int32), H, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="one word per row"):
        A.append_tree_attention(qkv, cu, past, kvp, mask[:3], H, Hkv, Hkv * 64, True)
    with pytest.raises(RuntimeError, match="max_seqlen_q=65"):
        A.append_tree_attention(qkv, cu, past, kvp, mask, H, Hkv, Hkv * 64, True, max_seqlen_q=65)
    with pytest.raises(RuntimeError, match="head counts"):
        A.append_tree_attention(qkv, cu, past, kvp, mask, H, 3, 3 * 64, True)
    with pytest.raises(RuntimeError, match="max_accept=65"):
        A.commit_path(kvp, past, torch.zeros((1, 65), dtype=torch.int32, device=d), torch.zeros((1,), dtype=torch.int32, device=d), Hkv,
                      Hkv * 64, True)
    with pytest.raises(RuntimeError, match="size_per_token"):
        A.commit_path(kvp, past, torch.zeros((1, 4), dtype=torch.int32, device=d), torch.zeros((1,), dtype=torch.int32, device=d), Hkv,
                      Hkv * 128, True)


def test_tree_attention_entry_validates_before_any_device_call(built_lib):
    from qserve_amd._lib import lib

    def call(qkv=16, out=32, cu=1, past=1, kvp=1, mask=8, T=4, B=1, msq=4, mb=2, H=8, Hkv=2, dh=128, qs=12 * 128, os_=8 * 128, tpb=64,
             spt=2 * 64, int4=1, zeros=1, max_past=-1, splits=1):
        return lib.qs_append_tree_attention(qkv, out, cu, past, kvp, mask, T, B, msq, mb, H, Hkv, dh, qs, os_, tpb, spt, int4, zeros, max_past,
                                            splits, None)

    for null in ("qkv", "out", "cu", "past", "kvp", "mask"):
        assert call(**{null: 0}) == -1 and b"null" in lib.qs_last_error()
    assert call(mask=4) == -1 and b"8-byte" in lib.qs_last_error()
    assert call(qkv=8) == -1 and call(qs=12 * 128 + 4) == -1             # misaligned qkv: the buffer, a row stride
    assert call(msq=65, T=65) == -1 and b"64" in lib.qs_last_error()      # a tree has at most 64 nodes per sequence
    assert call(H=8, Hkv=3) == -1 and b"head counts" in lib.qs_last_error()
    assert call(H=18, Hkv=2, qs=22 * 128, os_=18 * 128) == -2            # 9 query heads per KV head
    assert call(dh=64, qs=12 * 64, os_=8 * 64) == -2 and call(tpb=32) == -2 and call(zeros=0) == -2
    assert call(spt=2 * 128) == -1 and call(mb=0) == -1 and call(splits=-1) == -1
    assert call(T=0) == 0 and call(B=0) == 0 and call(msq=0) == 0        # nothing to do: no launch


def test_tree_writer_entry_validates_before_any_device_call(built_lib):
    from qserve_amd._lib import lib

    def call(qkv=16, cu=1, past=1, kvp=1, mask=8, T=4, B=1, mb=2, H=8, Hkv=2, tpb=64, spt=2 * 64, rot=128, int4=1, zeros=1):
        return lib.qs_append_tree_rope_update_kv_cache(qkv, cu, past, kvp, mask, T, B, mb, H, Hkv, tpb, spt, rot, 1e4, int4, zeros, None)

    for null in ("qkv", "cu", "past", "kvp", "mask"):
        assert call(**{null: 0}) == -1 and b"null" in lib.qs_last_error()
    assert call(qkv=8) == -1 and b"aligned" in lib.qs_last_error()       # misaligned qkv
    assert call(mask=4) == -1
    assert call(rot=64) == -2 and call(tpb=32) == -2 and call(zeros=0) == -2
    assert call(spt=100) == -1 and call(mb=0) == -1 and call(H=0) == -1 and call(Hkv=0) == -1
    assert call(T=0) == 0


def test_commit_entry_validates_before_any_device_call(built_lib):
    from qserve_amd._lib import lib

    def call(kvp=8, past=4, idx=4, lens=4, B=1, ma=4, mb=2, Hkv=2, tpb=64, spt=2 * 64, int4=1, zeros=1):
        return lib.qs_kv_cache_commit_path(kvp, past, idx, lens, B, ma, mb, Hkv, tpb, spt, int4, zeros, None)

    for null in ("kvp", "past", "idx", "lens"):
        assert call(**{null: 0}) == -1 and b"null" in lib.qs_last_error()
    assert call(ma=65) == -1 and b"64" in lib.qs_last_error()
    assert call(Hkv=0) == -1 and call(Hkv=3) == -1 and call(spt=2 * 128) == -1 and call(mb=0) == -1 and call(ma=-1) == -1
    assert call(tpb=32) == -2 and call(zeros=0) == -2
    assert call(B=0) == 0 and call(ma=0) == 0


@pytest.mark.parametrize("int4", [True, False], ids=["kv4", "kv8"])
def test_tree_oracle_with_chain_masks_is_the_append_composition(int4):
    """Chain words (2 << i) - 1: depth = index, visibility = the causal rule.  The float64 tree oracle then runs the statements of
    oracle.flash.attention_varlen on the same inputs; `expected` returns that result rounded to float32, so the comparison is made
    on the rounded values - where 1e-12 leaves room for nothing but equality."""
    H, Hkv = 6, 2
    r = np.random.default_rng(17 + int(int4))
    pasts, ns = [0, 70, 64, 5], [9, 64, 1, 0]
    B, W = len(pasts), (H + 2 * Hkv) * 128
    tables, nblocks = scattered_tables(r, B, 3)
    pool = kvattn.PagePool(nblocks, Hkv, 128, int4, fill=0xFF)
    for b, p in enumerate(pasts):
        if p:
            ctx = r.standard_normal((p, W)).astype(np.float16)
            kvattn.prefill_update_kv_cache(ctx, np.array([p]), kvattn.compute_padding_offsets(np.array([0, p], np.int32), p, p),
                                           tables[b:b + 1], pool, H, Hkv, p, BASE)
    new = r.standard_normal((sum(ns), W)).astype(np.float16)
    cu_q, past = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32), np.asarray(pasts, np.int32)
    words = [w for n in ns for w in chain_words(n)]
    rot = rotate_rows(new, cu_q, past, H, Hkv, BASE)
    assert np.array_equal(rotate_rows_tree(new, cu_q, past, words, H, Hkv, BASE).view(np.uint16), rot.view(np.uint16))
    ref = expected(rot, cu_q, past, tables, pool, H, Hkv)
    got = expected_tree(rot, cu_q, past, tables, pool, H, Hkv, words)
    assert got.dtype == np.float64 and np.abs(got.astype(np.float32).astype(np.float64) - ref.astype(np.float64)).max() <= 1e-12
    assert np.abs(got - ref).max() <= 1e-6          # (and un-rounded: within float32's rounding of the reference)
