"""The attention entries on the layouts their host checks ACCEPT but no call site of the engine produces: q / k / v / qkv / out
as views inside larger buffers - padded token strides (k and v in buffers of their own, with different strides), a leading row
offset and a leading element offset that keeps 16-byte (not 256-byte) alignment.

Every positive case asserts three things: (1) BIT-EQUALITY with the same call on contiguous copies of the same data - a layout
must not change a bit; (2) the float64 oracle at the bar of the entry's existing test (2e-3 prefill / append: test_flash_gpu.py,
test_append_gpu.py; 1e-3 decode: test_attention_gpu.py); (3) every byte outside the views untouched.  Inputs are surrounded by
fp16 NaN (nothing legal reads it: a wrong fetch shows as NaN or a large error), outputs by 0xA5 canary bytes.

Sequences of several FULL 64-key tiles matter: the tile stager of qserve_amd/csrc/flash_tile.h derives the K offsets of a full
tile from one register per lane, which only serves token strides that are multiples of 128 elements (other strides take the
per-piece offsets of its ragged path) - sequences under 64 keys never reach that code."""
import functools

import numpy as np
import pytest
import torch

import _attn_cases as AC
from _append_cases import expected, host_pool, scattered_tables
from _helpers import DevPools, dev
from oracle import flash as oflash
from oracle import kvattn, synth

pytestmark = pytest.mark.gpu
PREFILL_TOL = 2e-3      # tests/test_flash_gpu.py TOL
APPEND_TOL = 2e-3       # tests/test_append_gpu.py TOL
DECODE_TOL = 1e-3       # tests/test_attention_gpu.py TOL
NAN16, CANARY16 = 0x7E00, 0xA5A5
BASE = 1e4
ROPE = 5e5


class Padded:
    """A [rows, width] fp16 view inside a larger device buffer: token stride `stride` (elements), `row_off` rows and `elem_off`
    elements in front of it, a row of slack behind it.  poison = "nan": an input (every other half is a NaN); "canary": an output
    (the view included starts as 0xA5 bytes; only the view may change)."""

    def __init__(self, rows, width, stride, row_off, elem_off, device, poison="nan", align=8):
        assert stride >= width and elem_off % align == 0
        self.rows, self.width, self.stride = rows, width, stride
        self.fill = NAN16 if poison == "nan" else CANARY16 - 0x10000      # (as a signed 16-bit pattern)
        self.start = row_off * stride + elem_off
        total = self.start + (rows + 1) * stride
        self.raw = torch.full((total,), self.fill, dtype=torch.int16, device=device)
        self.view = self.raw.view(torch.float16).as_strided((rows, width), (stride, 1), self.start)
        inside = torch.zeros(total, dtype=torch.bool, device=device)
        inside.as_strided((rows, width), (stride, 1), self.start).fill_(True)
        self.outside = ~inside
        assert self.view.data_ptr() % (2 * align) == 0
        if elem_off:
            assert self.view.data_ptr() % 256 != 0, "the case is meant to leave the allocator's alignment"

    def load(self, data):
        self.view.copy_(data if isinstance(data, torch.Tensor) else dev(data, self.raw.device))
        self.snapshot = self.raw.clone()
        return self

    def heads(self, h):
        """[rows, h, 128] view (contiguous heads, padded token stride)."""
        assert self.width == h * 128
        return self.view.as_strided((self.rows, h, 128), (self.stride, 128, 1), self.view.storage_offset())

    def ptr(self):
        return self.view.data_ptr()

    def assert_untouched(self, what):
        """input: not a byte of the whole buffer changed"""
        assert torch.equal(self.raw, self.snapshot), f"{what}: the call wrote into an input buffer"

    def assert_padding_intact(self, what):
        """output: every half outside the view still holds the canary"""
        assert bool((self.raw[self.outside] == self.fill).all()), f"{what}: a byte outside the view was written"


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint16)


@pytest.fixture(params=[0, 1], ids=["round6", "rounds2to5"])
def flash_variant(request):
    """Both key loops of the prefill provider (as in tests/test_flash_gpu.py)."""
    from qserve_amd._lib import lib
    assert lib.qs_debug_flash_variant(request.param) == 0
    yield request.param
    lib.qs_debug_flash_variant(0)


# ---- prefill provider --------------------------------------------------------------------------------------------------------
LENS_FULL = [1, 63, 64, 65, 200, 300]      # full 64-key tiles with ragged tails, varlen neighbours on both sides
LENS_SHORT = [1, 17, 63, 40, 62]           # every sequence under one tile: the ragged path only


@functools.lru_cache(maxsize=None)
def _prefill_data(H, Hkv, lens, causal, seed):
    r = np.random.default_rng(seed)
    T = int(sum(lens))
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    q = r.standard_normal((T, H, 128)).astype(np.float16)
    k = r.standard_normal((T, Hkv, 128)).astype(np.float16)
    v = r.standard_normal((T, Hkv, 128)).astype(np.float16)
    return q, k, v, cu, oflash.attention_varlen(q, k, v, cu, cu, causal=causal)


def _prefill_padded(gpu, q, k, v, H, Hkv, kpad, vpad, qpad, offsets=True):
    """q, k, v numpy [T, heads, 128] -> three Padded inputs in three buffers (different strides, row and element offsets)."""
    Tq, Tk = q.shape[0], k.shape[0]
    ro, eo = zip(*(((2, 24), (3, 8), (1, 16)) if offsets else ((0, 0),) * 3))      # (row, element) offsets of q, k, v
    pq = Padded(Tq, H * 128, H * 128 + qpad, ro[0], eo[0] if qpad else 0, gpu).load(q.reshape(Tq, -1))
    pk = Padded(Tk, Hkv * 128, Hkv * 128 + kpad, ro[1], eo[1], gpu).load(k.reshape(Tk, -1))
    pv = Padded(Tk, Hkv * 128, Hkv * 128 + vpad, ro[2], eo[2], gpu).load(v.reshape(Tk, -1))
    return pq, pk, pv


def _prefill_shim_case(gpu, H, Hkv, lens, causal, kpad, vpad, qpad=8):
    from flash_attn.flash_attn_interface import flash_attn_varlen_func
    q, k, v, cu, ref = _prefill_data(H, Hkv, tuple(lens), causal, 100 * H + Hkv)
    mx = int(max(lens))
    packed = flash_attn_varlen_func(dev(q), dev(k), dev(v), dev(cu), dev(cu), mx, mx, dropout_p=0.0, causal=causal)
    pq, pk, pv = _prefill_padded(gpu, q, k, v, H, Hkv, kpad, vpad, qpad)
    out = flash_attn_varlen_func(pq.heads(H), pk.heads(Hkv), pv.heads(Hkv), dev(cu), dev(cu), mx, mx, dropout_p=0.0, causal=causal)
    torch.cuda.synchronize()
    err = np.abs(out.cpu().numpy().astype(np.float32) - ref)
    bad = int((_bits(out) != _bits(packed)).sum())
    print(f"prefill H={H} Hkv={Hkv} causal={causal} K pad {kpad} V pad {vpad} Q pad {qpad}: max abs err {np.nanmax(err):.3e}, "
          f"{bad} halves differ from the packed call, {int(np.isnan(err).sum())} NaN")
    assert bad == 0, f"{bad} output halves differ from the call on contiguous copies"
    assert np.isfinite(out.cpu().numpy()).all() and err.max() <= PREFILL_TOL, f"max abs err {err.max():.2e}"
    for p, n in ((pq, "q"), (pk, "k"), (pv, "v")):
        p.assert_untouched(n)


@pytest.mark.parametrize("kpad", [8, 64, 128])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 4), (8, 1)])
def test_prefill_padded_k_in_buffers_of_their_own(gpu, flash_variant, H, Hkv, causal, kpad):
    """K padded by 8 / 64 / 128 elements, V in another buffer with another stride, Q padded by 8, every base offset by rows and by
    a few 16-byte units.  (K strides that are no multiple of 128 fetched wrong chunks of every full tile before the stager's
    fallback; +128 was always right.)"""
    _prefill_shim_case(gpu, H, Hkv, LENS_FULL, causal, kpad=kpad, vpad={8: 72, 64: 8, 128: 24}[kpad])


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_prefill_padded_sequences_under_one_tile(gpu, flash_variant, causal):
    _prefill_shim_case(gpu, 8, 2, LENS_SHORT, causal, kpad=8, vpad=72)


@pytest.mark.parametrize("name", ["needle:4:eq", "needle:8:br"])
def test_prefill_planted_needles_on_a_padded_layout(gpu, flash_variant, name):
    """Two of the planted-needle cases of tests/_attn_cases.py (one key decides the output: a wrong 16-byte chunk of it moves the
    rows that see it by >= 50 x the bar) with K padded by 8, V by 64 and Q by 8 elements."""
    from flash_attn.flash_attn_interface import flash_attn_varlen_func
    sp = AC.prefill(name)
    c = sp["c"]
    H, Hkv = c["H"], c["Hkv"]
    pq, pk, pv = _prefill_padded(gpu, c["q"], c["k"], c["v"], H, Hkv, 8, 64, 8)
    lq, lk = np.diff(c["cu_q"]), np.diff(c["cu_k"])
    assert abs(c["scale"] - 1.0 / np.sqrt(128.0)) < 1e-12 and sp.get("rows") is None
    args = (dev(c["cu_q"]), dev(c["cu_k"]), int(lq.max()), int(lk.max()))
    out = flash_attn_varlen_func(pq.heads(H), pk.heads(Hkv), pv.heads(Hkv), *args, dropout_p=0.0, causal=sp["causal"])
    packed = flash_attn_varlen_func(dev(c["q"]), dev(c["k"]), dev(c["v"]), *args, dropout_p=0.0, causal=sp["causal"])
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(packed)), "output differs from the call on contiguous copies"
    o = out.cpu().numpy().astype(np.float64)
    err = np.abs(o - AC.to_tokens(c, sp["ref"]))
    assert np.isfinite(o).all() and err.max() <= AC.PREFILL_BAR, f"max abs err {err.max():.2e}"
    for p, n in ((pq, "q"), (pk, "k"), (pv, "v")):
        p.assert_untouched(n)


@pytest.mark.parametrize("opad,ooff,why", [(8, 8, "whole rows, padding between them"), (4, 0, "8-byte stores: stride % 8 != 0"),
                                           (8, 4, "8-byte stores: base 8- but not 16-byte aligned")],
                         ids=["rows+8", "stride+4", "base+8B"])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_prefill_out_layouts_through_the_c_abi(gpu, flash_variant, causal, opad, ooff, why):
    """`out` with a padded token stride (the shim always allocates a contiguous one): H*128 + 8 keeps the whole-row stores of the
    round-6 kernel, H*128 + 4 and a base that is only 8-byte aligned take its 8-byte store path.  K and V stay padded as above."""
    from flash_attn.flash_attn_interface import flash_attn_varlen_func
    from qserve_amd._lib import lib
    H, Hkv = 8, 2
    q, k, v, cu, ref = _prefill_data(H, Hkv, tuple(LENS_FULL), causal, 100 * H + Hkv)
    T, mx = q.shape[0], max(LENS_FULL)
    packed = flash_attn_varlen_func(dev(q), dev(k), dev(v), dev(cu), dev(cu), mx, mx, dropout_p=0.0, causal=causal)
    pq, pk, pv = _prefill_padded(gpu, q, k, v, H, Hkv, 8, 72, 8)
    po = Padded(T, H * 128, H * 128 + opad, 2, ooff, gpu, poison="canary", align=4)
    assert po.ptr() % 16 == (8 if ooff % 8 else 0)
    cu_d = dev(cu)
    rc = lib.qs_flash_attn_varlen_fwd(pq.ptr(), pk.ptr(), pv.ptr(), po.ptr(), cu_d.data_ptr(), cu_d.data_ptr(), len(LENS_FULL), H, Hkv,
                                      128, pq.stride, pk.stride, pv.stride, po.stride, mx, mx, 1.0 / np.sqrt(128.0), int(causal), None)
    assert rc == 0, lib.qs_last_error()
    torch.cuda.synchronize()
    got = po.view.reshape(T, H, 128)
    assert np.array_equal(_bits(got), _bits(packed)), f"{why}: output differs from the contiguous call"
    err = np.abs(got.cpu().numpy().astype(np.float32) - ref)
    assert err.max() <= PREFILL_TOL, f"max abs err {err.max():.2e}"
    po.assert_padding_intact(why)
    for p, n in ((pq, "q"), (pk, "k"), (pv, "v")):
        p.assert_untouched(n)


# ---- append attention --------------------------------------------------------------------------------------------------------
APPEND_BATCH = ([0, 65, 1024, 65, 0, 1024, 65], [130, 200, 150, 0, 1, 33, 64])     # n >= 130: full tiles of new keys; 0, 1, 33 next to them
APPEND_SHORT = ([0, 65, 1024, 65], [63, 40, 1, 0])                                 # new keys under one tile everywhere


@functools.lru_cache(maxsize=None)
def _append_case(int4, which):
    """The cache filled, the writer run on the CONTIGUOUS qkv buffer, the contiguous attention call and the oracle - once per
    cache type; the padded layouts re-use the rotated rows and the pages (the attention does not write pages)."""
    from qserve_amd import append as A
    from qserve_backend import fused_attention as fa
    gpu = torch.device("cuda:0")
    pasts, ns = APPEND_BATCH if which == "full" else APPEND_SHORT
    H, Hkv = 8, 2
    spt = Hkv * (64 if int4 else 128)
    r = np.random.default_rng(17 + int(int4))
    B, W = len(pasts), (H + 2 * Hkv) * 128
    mb = (max(p + n for p, n in zip(pasts, ns)) + 63) // 64 + 1
    tables, nblocks = scattered_tables(r, B, mb)
    pools = DevPools(nblocks, Hkv, int4, gpu)
    kvp = pools.pointers(tables)
    live = [b for b in range(B) if pasts[b] > 0]
    lens = [pasts[b] for b in live]
    ctx = dev(r.standard_normal((sum(lens), W)).astype(np.float16))
    cu_ctx = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    fa.apply_bias_rope_update_kv_cache(ctx, dev(np.asarray(lens, np.int32)), fa.compute_padding_offsets(dev(cu_ctx), max(lens), sum(lens)),
                                       pools.pointers(tables[live]), H, Hkv, max(lens), 64, spt, 128, BASE, 8192, True, int4, True)
    T = int(sum(ns))
    cu_q = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    past = np.asarray(pasts, np.int32)
    qkv = dev(r.standard_normal((T, W)).astype(np.float16))
    A.append_rope_update_kv_cache(qkv, dev(cu_q), dev(past), kvp, H, Hkv, spt, BASE, int4)
    packed = A.append_attention(qkv, dev(cu_q), dev(past), kvp, H, Hkv, spt, int4, max_seqlen_q=int(max(ns)))
    torch.cuda.synchronize()
    hp = host_pool(pools.k.cpu().numpy(), pools.v.cpu().numpy(), Hkv, int4)
    ref = expected(qkv.cpu().numpy(), cu_q, past, tables, hp, H, Hkv)
    return dict(H=H, Hkv=Hkv, spt=spt, T=T, W=W, mb=mb, B=B, msq=int(max(ns)), cu_q=dev(cu_q), past=dev(past), kvp=kvp, pools=pools,
                pages=(pools.k.clone(), pools.v.clone()), qkv=qkv, packed=packed, ref=ref)


def _append_layout(gpu, int4, which, pad):
    from qserve_amd._lib import lib
    c = _append_case(int4, which)
    H, T, W = c["H"], c["T"], c["W"]
    pq = Padded(T, W, W + pad, 2, 8, gpu).load(c["qkv"])
    po = Padded(T, H * 128, H * 128 + 8, 1, 16, gpu, poison="canary")
    rc = lib.qs_append_attention(pq.ptr(), po.ptr(), c["cu_q"].data_ptr(), c["past"].data_ptr(), c["kvp"].data_ptr(), T, c["B"],
                                 c["msq"], c["mb"], H, c["Hkv"], 128, pq.stride, po.stride, 64, c["spt"], int(int4), 1, None)
    assert rc == 0, lib.qs_last_error()
    torch.cuda.synchronize()
    got = po.view.reshape(T, H, 128)
    err = np.abs(got.cpu().numpy().astype(np.float32) - c["ref"])
    bad = int((_bits(got) != _bits(c["packed"])).sum())
    print(f"append {'kv4' if int4 else 'kv8'} {which} qkv pad {pad}: max abs err {np.nanmax(err):.3e}, {bad} halves differ from the "
          f"packed call, {int(np.isnan(err).sum())} NaN")
    assert bad == 0, f"{bad} output halves differ from the call on the contiguous buffer"
    assert np.isfinite(got.cpu().numpy()).all() and err.max() <= APPEND_TOL, f"max abs err {err.max():.2e}"
    po.assert_padding_intact("out")
    pq.assert_untouched("qkv")
    assert torch.equal(c["pools"].k, c["pages"][0]) and torch.equal(c["pools"].v, c["pages"][1]), "the attention wrote a page"


@pytest.mark.parametrize("pad", [8, 64, 128])
@pytest.mark.parametrize("int4", [True, False], ids=["kv4", "kv8"])
def test_append_padded_qkv_and_out(gpu, int4, pad):
    """qkv_stride0 = W + 8 / + 64 / + 128 and out_stride0 = H*128 + 8 through the C ABI, past in {0, 65, 1024}, n >= 130 next to
    n in {0, 1, 33}.  (The first two strides fetched wrong K chunks of every full tile of new keys before the stager's fallback.)"""
    _append_layout(gpu, int4, "full", pad)


@pytest.mark.parametrize("int4", [True, False], ids=["kv4", "kv8"])
def test_append_padded_new_keys_under_one_tile(gpu, int4):
    _append_layout(gpu, int4, "short", 8)


# ---- decode --------------------------------------------------------------------------------------------------------------------
DECODE_PLANS = {"default": 0, "valu": 1, "split3": 103}


def _decode_setup(gpu, int4, seed=23):
    import qserve_backend.fused_attention as fa
    B, H, Hkv, lengths = 5, 8, 2, [1, 65, 130, 700, 1536]
    pr = synth.attention_problem(B, H, Hkv, lengths, seed=seed)
    opool = kvattn.PagePool(pr["nblocks"], Hkv, 128, int4, fill=0xFF)
    seq = (pr["lengths"] - 1).astype(np.int32)
    hist = np.concatenate(pr["hist"])
    cu = np.concatenate([[0], np.cumsum(seq)]).astype(np.int32)
    mx = int(seq.max())
    kvattn.prefill_update_kv_cache(hist.copy(), seq, kvattn.compute_padding_offsets(cu, mx, hist.shape[0]), pr["tables"], opool, H, Hkv,
                                   mx, ROPE)
    ref = kvattn.decode_attention(pr["q"], pr["k"], pr["v"], pr["tables"], pr["lengths"], opool, ROPE, "exact")   # (updates opool)

    def fresh():
        pools = DevPools(pr["nblocks"], Hkv, int4, gpu)
        fa.apply_bias_rope_update_kv_cache(dev(hist), dev(seq), fa.compute_padding_offsets(dev(cu), mx, hist.shape[0]),
                                           pools.pointers(pr["tables"]), H, Hkv, mx, 64, Hkv * (64 if int4 else 128), 128, ROPE, 8192,
                                           True, int4, True)
        return pools
    return pr, opool, ref, fresh, (B, H, Hkv)


def _decode_views(gpu, pr, B, H, Hkv):
    """q, k, v in three buffers: q with a stride of its own, k and v with the ONE kv_stride0 of the entry but different row and
    element offsets."""
    pq = Padded(B, H * 128, H * 128 + 8, 2, 24, gpu).load(pr["q"].reshape(B, -1))
    pk = Padded(B, Hkv * 128, Hkv * 128 + 24, 3, 8, gpu).load(pr["k"].reshape(B, -1))
    pv = Padded(B, Hkv * 128, Hkv * 128 + 24, 1, 16, gpu).load(pr["v"].reshape(B, -1))
    return pq, pk, pv


@pytest.mark.parametrize("plan", DECODE_PLANS)
@pytest.mark.parametrize("int4", [True, False], ids=["kv4", "kv8"])
def test_decode_padded_q_k_v(gpu, int4, plan):
    import qserve_backend.fused_attention as fa
    from qserve_amd._lib import lib
    pr, opool, ref, fresh, (B, H, Hkv) = _decode_setup(gpu, int4)
    spt = Hkv * (64 if int4 else 128)
    args = (dev(pr["lengths"]), None, 8192, 64, spt, int(pr["lengths"].max()), 128, ROPE, True, int4, True)
    pq, pk, pv = _decode_views(gpu, pr, B, H, Hkv)
    lib.qs_set_attention_variant(DECODE_PLANS[plan])
    try:
        p1 = fresh()
        packed = fa.single_query_attention(dev(pr["q"]), dev(pr["k"]), dev(pr["v"]), p1.pointers(pr["tables"]), *args)
        p2 = fresh()
        out = fa.single_query_attention(pq.heads(H), pk.heads(Hkv), pv.heads(Hkv), p2.pointers(pr["tables"]), *args)
        torch.cuda.synchronize()
    finally:
        lib.qs_set_attention_variant(0)
    assert np.array_equal(_bits(out), _bits(packed)), "output differs from the call on contiguous copies"
    assert torch.equal(p2.k, p1.k) and torch.equal(p2.v, p1.v), "cache pages differ from the call on contiguous copies"
    for p, n in ((pq, "q"), (pk, "k"), (pv, "v")):
        p.assert_untouched(n)
    o = out.cpu().numpy().astype(np.float32)
    long_rows = pr["lengths"] >= 64                      # (test_attention_gpu.run_case: the plain bar on realistic contexts)
    if plan != "valu":                                   # (the VALU kernel's reference is the fp16-cache oracle: test_attn_peaked_gpu.py)
        assert np.array_equal(p2.k.cpu().numpy(), opool.k) and np.array_equal(p2.v.cpu().numpy(), opool.v), "pages differ from the oracle's"
        err = np.abs(o - ref.astype(np.float32))[long_rows]
        assert np.isfinite(o).all() and err.max() <= DECODE_TOL, f"max abs err vs exact oracle {err.max():.2e}"


def test_decode_quant_entry_padded_q_k_v(gpu):
    """qs_single_query_attention_quant (KV4, the in-kernel finisher) once on the same views: fp16 output, int8 row, scale, row sum
    and pages bit for bit the packed call's."""
    from qserve_amd import fused
    pr, opool, ref, fresh, (B, H, Hkv) = _decode_setup(gpu, True)
    args = (8192, 64, Hkv * 64, int(pr["lengths"].max()), 128, ROPE, True, True, True)
    pq, pk, pv = _decode_views(gpu, pr, B, H, Hkv)
    res = []
    for q, k, v in ((dev(pr["q"]), dev(pr["k"]), dev(pr["v"])), (pq.heads(H), pk.heads(Hkv), pv.heads(Hkv))):
        pools = fresh()
        qo = torch.full((B, H * 128), 55, dtype=torch.int8, device=gpu)
        qs, qm = torch.full((B,), 5.0, dtype=torch.float16, device=gpu), torch.full((B,), 7.0, dtype=torch.float16, device=gpu)
        out = fused.single_query_attention_quant(q, k, v, pools.pointers(pr["tables"]), dev(pr["lengths"]), qo, qs, *args, quant_sum=qm)
        torch.cuda.synchronize()
        res.append((out, qo, qs, qm, pools))
    (o1, q1, s1, m1, p1), (o2, q2, s2, m2, p2) = res
    assert np.array_equal(_bits(o2), _bits(o1)) and torch.equal(q2, q1) and np.array_equal(_bits(s2), _bits(s1)) and \
        np.array_equal(_bits(m2), _bits(m1))
    assert torch.equal(p2.k, p1.k) and torch.equal(p2.v, p1.v)
    for p, n in ((pq, "q"), (pk, "k"), (pv, "v")):
        p.assert_untouched(n)
    err = np.abs(o2.cpu().numpy().astype(np.float32) - ref.astype(np.float32))[pr["lengths"] >= 64]
    assert err.max() <= DECODE_TOL, f"max abs err vs exact oracle {err.max():.2e}"


def test_decode_shim_refuses_k_and_v_with_different_strides(gpu):
    """The C entry has ONE kv_stride0: k and v views whose token strides differ cannot be expressed - an error, not v read at k's stride."""
    import qserve_backend.fused_attention as fa
    B, H, Hkv = 2, 8, 2
    q = torch.zeros((B, H, 128), dtype=torch.float16, device=gpu)
    k = torch.zeros((B, Hkv, 128), dtype=torch.float16, device=gpu)
    v = Padded(B, Hkv * 128, Hkv * 128 + 8, 0, 0, gpu).load(np.zeros((B, Hkv * 128), np.float16)).heads(Hkv)
    kvp = torch.zeros((B, 2, 2), dtype=torch.int64, device=gpu)
    with pytest.raises(RuntimeError, match="same token stride"):
        fa.single_query_attention(q, k, v, kvp, torch.ones((B,), dtype=torch.int32, device=gpu), None, 8192, 64, Hkv * 64, 1, 128, ROPE,
                                  True, True, True)
