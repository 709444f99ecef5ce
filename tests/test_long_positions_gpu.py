"""Positions and contexts far beyond the rest of the GPU suite: the three KV writers at positions up to 131 071 (bit-exact against the
numpy oracle, three RoPE bases), decode attention from 8 192 to 130 985 tokens (both matrix-core families up to 192 pages, the VALU
family behind them), and the append family - un-split, split-KV, tree, shared prefix - over 33 000 and 130 984 cached tokens.

The attention cases are the aliased construction of tests/_long_cases.py: its host conditions (an eighth of the context, and every
page range a launch uses as a split, decide the result at the bar) are asserted before the launches under test.  TOL is the 2e-3 of
tests/test_append_gpu.py, not loosened; every case prints a `LONGPOS` line with its measured maximum error
(profiles/long_positions.txt holds a run's lines).  The RoPE source of a call is read from qs_debug_rope_table_state and printed."""
import functools

import numpy as np
import pytest
import torch

import _attn_cases as AC
import _long_cases as LC
from _append_cases import host_pool, rotate_rows
from _helpers import DevPools, dev, rope_table_state
from _tree_cases import as_int64, chain_words, rotate_rows_tree, words_from_parents
from oracle import kvattn

pytestmark = pytest.mark.gpu
TOL = LC.TOL
KV = [pytest.param(True, id="kv4"), pytest.param(False, id="kv8")]
HEADS = [(8, 2), (8, 1)]
LENGTHS = [pytest.param(False, id="33000"), pytest.param(True, id="130984")]


def _np(t):
    return t.detach().cpu().numpy()


def _spt(Hkv, int4):
    return Hkv * (64 if int4 else 128)


def _prefill(rows, seq_len, kvp, H, Hkv, int4, base):
    """The existing prefill writer over ONE sequence of seq_len tokens (in place on rows and the pages)."""
    from qserve_backend import fused_attention as fa
    cu = dev(np.asarray([0, seq_len], np.int32))
    fa.apply_bias_rope_update_kv_cache(rows, dev(np.asarray([seq_len], np.int32)), fa.compute_padding_offsets(cu, seq_len, seq_len), kvp, H, Hkv,
                                       seq_len, 64, _spt(Hkv, int4), 128, base, 8192, True, int4, True)


def _canaried_rows(src, gpu):
    """fp16 rows on the device with 4 KiB of 0xA5 behind them -> (rows, check)."""
    nbytes = src.size * 2
    raw = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=gpu)
    rows = raw[:nbytes].view(torch.float16).view(*src.shape)
    rows.copy_(dev(src))

    def check():
        assert bool((raw[nbytes:] == 0xA5).all()), "write behind the qkv buffer"
    return rows, check


# =====================================================================================================================================
# 1. writers: only the positions are large
# =====================================================================================================================================
WH, WHKV, WMB = 8, 2, 2048
W_PASTS = [x - 2 for x in (2048, 8192, 12288, 32768, 65536)] + [131071 - 3]      # n = 4: four straddles and one sequence ending at 131 071
W_PARENTS = [-1, 0, 0, 1]                                                        # depths 0 1 1 2: not the node indices


def _writer_tables(rng):
    """Every entry that receives a token names a page of its own; all others the 0xFF-filled dummy page (last).  K and V permuted."""
    B = len(W_PASTS)
    pages = [sorted({(p + i) // 64 for i in range(4)}) for p in W_PASTS]
    real = sum(len(x) for x in pages)
    tab = np.full((B, 2, WMB), real, np.int64)
    perm_k, perm_v = rng.permutation(real), rng.permutation(real)
    i = 0
    for b, pg in enumerate(pages):
        for j in pg:
            tab[b, 0, j], tab[b, 1, j] = perm_k[i], perm_v[i]
            i += 1
    return tab, real + 1


def _expected_writer(src, rot, tables, nblocks, int4):
    """Rotated rows -> the oracle's pool: token i of sequence b quantised into slot past + i (K from the rotated row, V raw)."""
    pool = kvattn.PagePool(nblocks, WHKV, 128, int4, fill=0xFF)
    k = rot[:, WH * 128:(WH + WHKV) * 128].reshape(-1, WHKV, 128)
    v = src[:, (WH + WHKV) * 128:].reshape(-1, WHKV, 128)
    kb, ks, kz = kvattn.kv_quantize(k, int4)
    vb, vs, vz = kvattn.kv_quantize(v, int4)
    for b, p in enumerate(W_PASTS):
        for i in range(4):
            t, pos = 4 * b + i, p + i
            for h in range(WHKV):
                pool.write_token("k", int(tables[b, 0, pos // 64]), pos % 64, h, kb[t, h], ks[t, h], kz[t, h])
                pool.write_token("v", int(tables[b, 1, pos // 64]), pos % 64, h, vb[t, h], vs[t, h], vz[t, h])
    return pool


@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("base", [1e4, 5e5, 1e6])
def test_append_and_tree_writers_at_long_positions(gpu, base, int4):
    """Rotated rows, written slots (data, scale, zero), every other byte of the real pages and the dummy page, and a canary behind qkv:
    bit for bit.  Positions from 32 768 on are beyond every table (the length is clamped to 32 768): evaluated in the kernel."""
    from qserve_amd import append as A
    r = np.random.default_rng(int(base) % 1000 + int(int4))
    B, W = len(W_PASTS), (WH + 2 * WHKV) * 128
    tables, nblocks = _writer_tables(r)
    src = r.standard_normal((4 * B, W)).astype(np.float16)
    cu_q, past = np.arange(0, 4 * B + 1, 4, dtype=np.int32), np.asarray(W_PASTS, np.int32)
    chain = as_int64([w for _ in range(B) for w in chain_words(4)])
    tree = [w for _ in range(B) for w in words_from_parents(W_PARENTS)]
    before = rope_table_state(base)
    results = {}
    for name, words in (("append", None), ("chain", chain), ("tree", as_int64(tree))):
        pools = DevPools(nblocks, WHKV, int4, gpu)
        rows, check = _canaried_rows(src, gpu)
        if words is None:
            A.append_rope_update_kv_cache(rows, dev(cu_q), dev(past), pools.pointers(tables), WH, WHKV, _spt(WHKV, int4), base, int4)
        else:
            A.append_tree_rope_update_kv_cache(rows, dev(cu_q), dev(past), pools.pointers(tables), dev(words), WH, WHKV, _spt(WHKV, int4), base,
                                               int4)
        torch.cuda.synchronize()
        check()
        results[name] = (_np(rows).copy(), _np(pools.k), _np(pools.v))
    after = rope_table_state(base)
    print(f"writers base {base:g} int4={int4}: RoPE tables (slots, rows for this base) before {before} after {after}")
    assert after[1] <= 32768 < max(W_PASTS), "positions >= 32 768 cannot come from a table"
    assert after[1] >= before[1] and after[0] >= before[0]
    lin = rotate_rows(src, cu_q, past, WH, WHKV, base)
    for name, rot in (("append", lin), ("chain", lin), ("tree", rotate_rows_tree(src, cu_q, past, tree, WH, WHKV, base))):
        rows, pk, pv = results[name]
        want = _expected_writer(src, rot, tables, nblocks, int4)
        assert np.array_equal(rows.view(np.uint16), rot.view(np.uint16)), f"{name}: rotated rows differ from the oracle"
        assert np.array_equal(pk, want.k), f"{name}: K pages differ from the oracle (written slots, or bytes that should keep the fill)"
        assert np.array_equal(pv, want.v), f"{name}: V pages differ from the oracle"
        assert (pk[-1] == 0xFF).all() and (pv[-1] == 0xFF).all(), f"{name}: the dummy page was written"
    assert not np.array_equal(results["tree"][0], results["append"][0]), "the tree's depths must differ from the node indices"


@pytest.mark.parametrize("int4", KV)
def test_prefill_writer_beyond_the_table_clamp(gpu, int4):
    """seq_len = 32 770 > 32 768: no table can cover the request, the per-lane form runs.  Sampled rows against the oracle, and every
    row and page against the append writer run on the same tokens in chunks."""
    from qserve_amd import append as A
    base, S, H, Hkv = 1e6, 32770, 1, 1
    r = np.random.default_rng(17 + int(int4))
    W, mb = (H + 2 * Hkv) * 128, (S + 63) // 64
    src = r.standard_normal((S, W)).astype(np.float16)
    tables = np.stack([r.permutation(mb), r.permutation(mb)])[None].astype(np.int64)
    pools, pools2 = DevPools(mb + 1, Hkv, int4, gpu), DevPools(mb + 1, Hkv, int4, gpu)
    rows, check = _canaried_rows(src, gpu)
    before = rope_table_state(base)
    _prefill(rows, S, pools.pointers(tables), H, Hkv, int4, base)
    torch.cuda.synchronize()
    after = rope_table_state(base)
    print(f"prefill writer seq_len {S} int4={int4}: RoPE tables before {before} after {after}")
    assert before[1] < S and after[1] < S, "no table covers the request: the per-lane form ran"
    check()
    sample = [0, 1, 32766, 32767, 32768, 32769]
    got, hp = _np(rows), host_pool(_np(pools.k), _np(pools.v), Hkv, int4)
    for pos in sample:
        qk = kvattn.rope_neox(src[pos, :(H + Hkv) * 128].reshape(H + Hkv, 128), pos, base)
        assert np.array_equal(got[pos, :(H + Hkv) * 128].view(np.uint16), qk.reshape(-1).view(np.uint16)), f"row {pos}: rotated q / k"
        assert np.array_equal(got[pos, (H + Hkv) * 128:], src[pos, (H + Hkv) * 128:]), f"row {pos}: v changed"
        for which, x, t in (("k", qk[H:], 0), ("v", src[pos, (H + Hkv) * 128:].reshape(Hkv, 128), 1)):
            qb, qs, qz = kvattn.kv_quantize(x, int4)
            data, sc, zr = hp._views(hp.k if which == "k" else hp.v, int(tables[0, t, pos // 64]))
            assert np.array_equal(data[0, pos % 64], qb[0]) and sc[0, pos % 64].view(np.uint16) == qs[0].view(np.uint16) and \
                zr[0, pos % 64].view(np.uint16) == qz[0].view(np.uint16), f"row {pos}: {which} slot"
    rows2 = dev(src)
    kvp2 = pools2.pointers(tables)
    for s in range(0, S, 4096):
        n = min(4096, S - s)
        A.append_rope_update_kv_cache(rows2[s:s + n], dev(np.asarray([0, n], np.int32)), dev(np.asarray([s], np.int32)), kvp2, H, Hkv,
                                      _spt(Hkv, int4), base, int4)
    torch.cuda.synchronize()
    assert torch.equal(rows2, rows), "prefill writer and chunked append writer: rotated rows differ"
    assert torch.equal(pools2.k, pools.k) and torch.equal(pools2.v, pools.v), "prefill writer and chunked append writer: pages differ"
    assert bool((pools.k[mb] == 0xFF).all()) and bool((pools.v[mb] == 0xFF).all())


# =====================================================================================================================================
# 2. the aliased long context on the device
# =====================================================================================================================================
class _Dev:
    """The case's pools on the device: 0xFF everywhere, the 8 + B history pages written by the existing prefill writer."""

    def __init__(self, case, gpu, base):
        self.pools = DevPools(case.nblocks, case.Hkv, case.int4, gpu)
        _prefill(dev(case.hist), case.hist_len, self.pools.pointers(case.hist_tables), case.H, case.Hkv, case.int4, base)
        self.kvp = self.pools.pointers(case.tables)
        torch.cuda.synchronize()


def _host(d, case):
    return host_pool(_np(d.pools.k), _np(d.pools.v), case.Hkv, case.int4)


def _report(what, got, ref):
    got = _np(got).astype(np.float32)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = float(np.abs(got - ref).max())
    print(f"LONGPOS {what}: max abs err {err:.3e}")
    return err


# ---- decode -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("L", [8192, 8193, 12288, 12289, 32769, LC.LONGEST + 1])
def test_decode_attention_at_long_contexts(gpu, L, int4):
    from qserve_amd.plan import attention_plan
    from qserve_backend import fused_attention as fa
    case = LC.decode_case(int4, L)
    H, Hkv, B, base = case.H, case.Hkv, case.B, LC.BASE
    plan = attention_plan(B, H, Hkv, case.mb, L, int4)
    assert plan["family"] == ("valu" if case.mb > 192 else "mfma_kv4" if int4 else "mfma_kv8"), plan
    d = _Dev(case, gpu, base)
    hp = _host(d, case)
    rot = rotate_rows(case.new, case.cu_q, case.past, H, Hkv, base)
    refs, ref = LC.references(case, rot, hp)
    sets = [LC.decode_split_ranges(int(p), plan["kv_splits"], int4) if plan["kv_splits"] > 1 else [] for p in case.past]
    LC.conditions(case, refs, sets, f"decode L={L} int4={int4}", AC.SENS)
    new = dev(case.new)
    q, k, v = [x.reshape(B, -1, 128) for x in new.split([H * 128, Hkv * 128, Hkv * 128], dim=-1)]
    before = rope_table_state(base)
    out = fa.single_query_attention(q, k, v, d.kvp, dev(case.past + 1), None, 8192, 64, case.spt, L, 128, base, True, int4, True)
    torch.cuda.synchronize()
    print(f"decode L={L} int4={int4} {plan}: RoPE tables (slots, rows for base {base:g}) before {before} after {rope_table_state(base)}")
    # the new token's slot, bit for bit; every other byte as it was
    kb, ks, kz = kvattn.kv_quantize(rot[:, H * 128:(H + Hkv) * 128].reshape(B, Hkv, 128), int4)
    vb, vs, vz = kvattn.kv_quantize(case.new[:, (H + Hkv) * 128:].reshape(B, Hkv, 128), int4)
    for b in range(B):
        pos = int(case.past[b])
        for h in range(Hkv):
            hp.write_token("k", int(case.tables[b, 0, pos // 64]), pos % 64, h, kb[b, h], ks[b, h], kz[b, h])
            hp.write_token("v", int(case.tables[b, 1, pos // 64]), pos % 64, h, vb[b, h], vs[b, h], vz[b, h])
    assert np.array_equal(_np(d.pools.k), hp.k) and np.array_equal(_np(d.pools.v), hp.v), "pages: the new token's slot, or a byte elsewhere"
    err = _report(f"decode {plan['family']} L={L} int4={int4} B={B} splits={plan['kv_splits']}", out, ref)
    assert err <= TOL, f"max abs err {err:.2e}"


# ---- the append family ----------------------------------------------------------------------------------------------------------------
TREE = [-1, 0, 0, 1, 1, 2, -1, 6]      # per sequence: two roots, depths 0 1 1 2 2 2 0 1


@functools.lru_cache(maxsize=None)
def _append(H, Hkv, int4, longest):
    """Pools, both writers run on the new rows (the linear rows against the oracle), the float64 reference of the linear rows and the
    host conditions for every split set the tests below use - once per configuration; the attention never writes a page."""
    from qserve_amd import append as A
    from qserve_amd.plan import append_attention_split_plan
    gpu = torch.device("cuda:0")
    case = LC.append_case(H, Hkv, int4, longest)
    d = _Dev(case, gpu, LC.BASE)
    cu_q, past = dev(case.cu_q), dev(case.past)
    qkv, tqkv = dev(case.new), dev(case.new)
    words = [w for _ in range(case.B) for w in words_from_parents(TREE)]
    masks = dev(as_int64(words))
    A.append_tree_rope_update_kv_cache(tqkv, cu_q, past, d.kvp, masks, H, Hkv, case.spt, LC.BASE, int4)
    A.append_rope_update_kv_cache(qkv, cu_q, past, d.kvp, H, Hkv, case.spt, LC.BASE, int4)
    torch.cuda.synchronize()
    rot = rotate_rows(case.new, case.cu_q, case.past, H, Hkv, LC.BASE)
    assert np.array_equal(_np(qkv).view(np.uint16), rot.view(np.uint16)), "append writer: rotated rows differ from the oracle"
    hp = _host(d, case)
    refs, ref = LC.references(case, rot, hp)
    plan = append_attention_split_plan(case.B, 8, int(case.past.max()), H, Hkv, int4)
    assert 1 < plan["splits"] <= 64, plan
    LC.conditions(case, refs, LC.append_split_sets(case, (plan["splits"],)), f"append H={H} Hkv={Hkv} int4={int4} past={int(case.past[0])}", AC.SENS)
    return dict(case=case, d=d, cu_q=cu_q, past=past, qkv=qkv, tqkv=tqkv, words=words, masks=masks, ref=ref, plan=plan, hp=hp,
                pages=(d.pools.k.clone(), d.pools.v.clone()), tag=f"H={H} Hkv={Hkv} int4={int4} past={int(case.past[0])}")


@functools.lru_cache(maxsize=None)
def _tree_ref(H, Hkv, int4, longest):
    c = _append(H, Hkv, int4, longest)
    case = c["case"]
    rot = rotate_rows_tree(case.new, case.cu_q, case.past, c["words"], H, Hkv, LC.BASE)
    assert np.array_equal(_np(c["tqkv"]).view(np.uint16), rot.view(np.uint16)), "tree writer: rotated rows differ from the oracle"
    return LC.references(case, rot, c["hp"], words=c["words"])[1]


def _twice(c, call, what, ref):
    """The call into a canaried `out`, once more into a fresh one: bit-equal, nothing outside `out`, no page written, the spare page
    untouched, and the maximum error against `ref`."""
    case, d = c["case"], c["d"]
    raw = torch.full((8192 + case.T * case.H * 256,), 0xA5, dtype=torch.uint8, device=d.pools.k.device)
    out = raw[4096:-4096].view(torch.float16).view(case.T, case.H, 128)
    call(out)
    again = call(None)
    torch.cuda.synchronize()
    assert bool((raw[:4096] == 0xA5).all()) and bool((raw[-4096:] == 0xA5).all()), f"{what}: write outside `out`"
    assert torch.equal(out, again), f"{what}: a second identical call differs"
    assert torch.equal(d.pools.k, c["pages"][0]) and torch.equal(d.pools.v, c["pages"][1]), f"{what}: the attention wrote a page"
    assert bool((d.pools.k[case.spare] == 0xFF).all()) and bool((d.pools.v[case.vperm[case.spare]] == 0xFF).all()), f"{what}: spare page written"
    return out, _report(f"{what} {c['tag']}", out, ref)


def _linear(c, **kw):
    from qserve_amd import append as A
    case = c["case"]
    return lambda out: A.append_attention(c["qkv"], c["cu_q"], c["past"], c["d"].kvp, case.H, case.Hkv, case.spt, case.int4, max_seqlen_q=8,
                                          out=out, **kw)


def _tree(c, rows, masks, **kw):
    from qserve_amd import append as A
    case = c["case"]
    return lambda out: A.append_tree_attention(rows, c["cu_q"], c["past"], c["d"].kvp, masks, case.H, case.Hkv, case.spt, case.int4,
                                               max_seqlen_q=8, out=out, **kw)


@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("longest", LENGTHS)
def test_append_attention_unsplit(gpu, longest, H, Hkv, int4):
    c = _append(H, Hkv, int4, longest)
    _, err = _twice(c, _linear(c), "append un-split", c["ref"])
    assert err <= TOL, f"max abs err {err:.2e}"


@pytest.mark.parametrize("splits", [0, 8, 64])
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("longest", LENGTHS)
def test_append_attention_split(gpu, longest, H, Hkv, int4, splits):
    """0: the planner's own count for the true maximum past (asserted in _append: more than one split), 8 and 64 forced."""
    c = _append(H, Hkv, int4, longest)
    kw = dict(max_past=int(c["case"].past.max())) if splits == 0 else dict(num_splits=splits)
    _, err = _twice(c, _linear(c, **kw), f"append split {splits or 'plan=%d' % c['plan']['splits']}", c["ref"])
    assert err <= TOL, f"max abs err {err:.2e}"


@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("longest", LENGTHS)
def test_tree_attention_with_chain_words_is_the_split_entry(gpu, longest, H, Hkv, int4):
    c = _append(H, Hkv, int4, longest)
    chain = dev(as_int64([w for _ in range(c["case"].B) for w in chain_words(8)]))
    for splits in (8, 64):
        lin = _linear(c, num_splits=splits)(None)
        out, err = _twice(c, _tree(c, c["qkv"], chain, num_splits=splits), f"tree chain split {splits}", c["ref"])
        assert torch.equal(out, lin), f"{splits} splits: chain words differ from the split entry"
        assert err <= TOL, f"max abs err {err:.2e}"


@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("longest", LENGTHS)
def test_tree_attention_with_a_real_tree(gpu, longest, H, Hkv, int4):
    c = _append(H, Hkv, int4, longest)
    ref = _tree_ref(H, Hkv, int4, longest)
    for kw, name in ((dict(), "un-split"), (dict(num_splits=8), "split 8")):
        _, err = _twice(c, _tree(c, c["tqkv"], c["masks"], **kw), f"tree {name}", ref)
        assert err <= TOL, f"{name}: max abs err {err:.2e}"


@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("longest", LENGTHS)
def test_append_attention_shared_prefix(gpu, longest, H, Hkv, int4):
    """The two sequences as one group sharing their first 256 pages; prefix and suffix cut into LC.SHARED_SPLITS ranges each."""
    from qserve_amd import append as A
    c = _append(H, Hkv, int4, longest)
    case = c["case"]
    assert np.array_equal(case.tables[0, :, :LC.SHARED_PAGES], case.tables[1, :, :LC.SHARED_PAGES])
    groups = A.shared_prefix_groups([2], [LC.SHARED_PAGES * 64], device=gpu, batch=2)

    def call(out):
        return A.append_attention_shared(c["qkv"], c["cu_q"], c["past"], c["d"].kvp, H, Hkv, case.spt, int4, groups, max_seqlen_q=8, out=out,
                                         max_group_tokens=16, num_prefix_splits=LC.SHARED_SPLITS, num_suffix_splits=LC.SHARED_SPLITS)
    _, err = _twice(c, call, "append shared 256 pages", c["ref"])
    assert err <= TOL, f"max abs err {err:.2e}"
