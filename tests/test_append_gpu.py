"""GPU parity of append attention (qserve_amd.append): the offset-aware writer bit for bit against the prefill writer, the
attention against the composition of the existing oracles (tests/_append_cases.py), the two corner cases against the ops they
generalise (past = 0: prefill pair, n = 1: decode), canaries, and DecodeEngine.prefill_chunked."""
import numpy as np
import pytest
import torch

from _append_cases import compose, expected, expected_rows, host_pool, rotate_rows, scattered_tables
from _helpers import DevPools, dev
from oracle import kvattn

pytestmark = pytest.mark.gpu
TOL = 2e-3      # the project's bar for an fp16 MFMA attention against a float64 oracle on standard normal inputs (test_flash_gpu.py)
BASE = 1e4
# G = H / Hkv = 4, 4, 1, 8 - and 3, 3, 5, 7, 2: where G does not divide 128 the 32 rows of a wave straddle tokens unevenly (tok_first,
# tok_last, need_mask, r < tq * G and the store mapping of append_attention.hip all depend on it)
HEADS = [(32, 8), (8, 2), (4, 4), (8, 1), (6, 2), (12, 4), (5, 1), (7, 1), (16, 8)]
KV = [pytest.param(True, id="kv4"), pytest.param(False, id="kv8")]


def _spt(Hkv, int4):
    return Hkv * (64 if int4 else 128)


def _prefill_write(qkv, lens, kvp, H, Hkv, int4):
    """The existing writer over whole sequences (in place on qkv and the pages)."""
    from qserve_backend import fused_attention as fa
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    mx = int(max(lens))
    pad = fa.compute_padding_offsets(dev(cu), mx, int(cu[-1]))
    fa.apply_bias_rope_update_kv_cache(qkv, dev(np.asarray(lens, np.int32)), pad, kvp, H, Hkv, mx, 64, _spt(Hkv, int4), 128, BASE,
                                       8192, True, int4, True)
    return cu


def _np(t):
    return t.detach().cpu().numpy()


class _Canaried:
    """out [T, H, 128] fp16 between two 4 KiB areas of 0xA5."""

    def __init__(self, T, H, device):
        self.raw = torch.full((8192 + T * H * 256,), 0xA5, dtype=torch.uint8, device=device)
        self.out = self.raw[4096:4096 + T * H * 256].view(torch.float16).view(T, H, 128)

    def check(self):
        assert bool((self.raw[:4096] == 0xA5).all()) and bool((self.raw[-4096:] == 0xA5).all()), "write outside `out`"


def _spare_blocks_untouched(pools, tables, nblocks):
    used_k, used_v = set(tables[:, 0].ravel().tolist()), set(tables[:, 1].ravel().tolist())
    for name, pool, used in (("K", pools.k, used_k), ("V", pools.v, used_v)):
        spare = [i for i in range(nblocks) if i not in used]
        assert spare and bool((pool[spare] == 0xFF).all()), f"a {name} page of no sequence was written"


# ---- 1. the writer, bit-exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_writer_in_ragged_chunks_equals_the_prefill_writer(gpu, H, Hkv, int4):
    from qserve_amd import append as A
    r = np.random.default_rng(7 * H + Hkv + int(int4))
    lens = [150, 64, 65, 1, 300]
    rounds = [[37, 64, 1, 1, 100], [27, 0, 64, 0, 92], [86, 0, 0, 0, 108]]     # cuts inside pages and on page boundaries
    assert [sum(c) for c in zip(*rounds)] == lens
    B, mb, W = len(lens), 6, (H + 2 * Hkv) * 128
    tables, nblocks = scattered_tables(r, B, mb)
    src = r.standard_normal((sum(lens), W)).astype(np.float16)
    cu_full = np.concatenate([[0], np.cumsum(lens)])

    whole, pools_w = dev(src), DevPools(nblocks, Hkv, int4, gpu)
    _prefill_write(whole, lens, pools_w.pointers(tables), H, Hkv, int4)

    pools_c, kvp = DevPools(nblocks, Hkv, int4, gpu), None
    kvp = pools_c.pointers(tables)
    rotated = np.zeros_like(src)
    done = np.zeros(B, np.int64)
    for ns in rounds:
        rows = np.concatenate([np.arange(cu_full[b] + done[b], cu_full[b] + done[b] + ns[b]) for b in range(B)]).astype(np.int64)
        chunk = dev(src[rows])
        cu_q = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
        A.append_rope_update_kv_cache(chunk, dev(cu_q), dev(done.astype(np.int32)), kvp, H, Hkv, _spt(Hkv, int4), BASE, int4)
        rotated[rows] = _np(chunk)
        done += ns
    torch.cuda.synchronize()
    assert np.array_equal(rotated.view(np.uint16), _np(whole).view(np.uint16)), "rotated qkv rows differ"
    assert torch.equal(pools_c.k, pools_w.k), "K pages differ"
    assert torch.equal(pools_c.v, pools_w.v), "V pages differ"
    # slots beyond each length keep the fill (data, scale and zero slots), and so do the pages of nobody
    hp = host_pool(_np(pools_c.k), _np(pools_c.v), Hkv, int4)
    for b, L in enumerate(lens):
        for which, pool in (("k", hp.k), ("v", hp.v)):
            for blk in range(L // 64, mb):
                data, sc, zr = hp._views(pool, tables[b, 0 if which == "k" else 1, blk])
                s0 = L - 64 * blk if blk == L // 64 else 0
                assert (data[:, s0:] == 0xFF).all() and (sc.view(np.uint16)[:, s0:] == 0xFFFF).all() and \
                    (zr.view(np.uint16)[:, s0:] == 0xFFFF).all(), f"sequence {b}: slot >= {L} written"
    _spare_blocks_untouched(pools_c, tables, nblocks)


# ---- 2. attention against the oracle composition --------------------------------------------------------------------------
def _run_case(gpu, H, Hkv, int4, pasts, ns, seed, rows=None, heads=None):
    """Fill the cache with `pasts` tokens per sequence (existing writer), run append() on `ns` new tokens, compare with the oracle
    composition.  -> (max abs error, context for further checks)."""
    from qserve_amd import append as A
    r = np.random.default_rng(seed)
    B, W = len(pasts), (H + 2 * Hkv) * 128
    mb = (max(p + n for p, n in zip(pasts, ns)) + 63) // 64 + 1
    tables, nblocks = scattered_tables(r, B, mb)
    pools = DevPools(nblocks, Hkv, int4, gpu)
    kvp = pools.pointers(tables)
    live = [b for b in range(B) if pasts[b] > 0]
    if live:
        ctx = dev(r.standard_normal((sum(pasts[b] for b in live), W)).astype(np.float16))
        _prefill_write(ctx, [pasts[b] for b in live], pools.pointers(tables[live]), H, Hkv, int4)
    T = int(sum(ns))
    new = r.standard_normal((T, W)).astype(np.float16)
    cu_q = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    past = np.asarray(pasts, np.int32)
    qkv = dev(new)
    box = _Canaried(T, H, gpu)
    A.append_rope_update_kv_cache(qkv, dev(cu_q), dev(past), kvp, H, Hkv, _spt(Hkv, int4), BASE, int4)
    out = A.append_attention(qkv, dev(cu_q), dev(past), kvp, H, Hkv, _spt(Hkv, int4), int4, max_seqlen_q=int(max(ns)), out=box.out)
    torch.cuda.synchronize()
    box.check()
    _spare_blocks_untouched(pools, tables, nblocks)
    got = _np(out).astype(np.float32)
    assert np.isfinite(got).all()
    rot = _np(qkv)
    assert np.array_equal(rot.view(np.uint16), rotate_rows(new, cu_q, past, H, Hkv, BASE).view(np.uint16))
    hp = host_pool(_np(pools.k), _np(pools.v), Hkv, int4)
    if rows is None:
        err = np.abs(got - expected(rot, cu_q, past, tables, hp, H, Hkv)).max()
    else:
        ref = expected_rows(rot, cu_q, past, tables, hp, H, Hkv, rows, heads)
        err = np.abs(got[np.asarray(rows)][:, np.asarray(heads)] - ref).max()
    print(f"append attention H={H} Hkv={Hkv} int4={int4} past={list(pasts)} n={list(ns)}: max abs err {err:.3e}")
    return err, dict(rot=rot, cu_q=cu_q, past=past, tables=tables, hp=hp, out=out)


@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_attention_ragged_batch_against_the_oracle_composition(gpu, H, Hkv, int4):
    pasts = [0, 1, 63, 64, 65, 200, 1024, 64, 200, 63, 1024, 0]
    ns = [300, 129, 64, 33, 32, 31, 7, 2, 1, 0, 33, 1]
    err, _ = _run_case(gpu, H, Hkv, int4, pasts, ns, seed=11 * H + Hkv + int(int4))
    assert err <= TOL, f"max abs err {err:.2e}"


@pytest.mark.parametrize("int4", KV)
def test_attention_llama3_8b_shape_sampled_rows(gpu, int4):
    """past 4096, n 512, Llama-3-8B heads; sampled (row, head) pairs: both ends of the chunk, around the 32-token query tiles and
    the 64-key tiles."""
    rows = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 300, 447, 448, 510, 511, 512, 513, 600, 1023]
    err, _ = _run_case(gpu, 32, 8, int4, [4096, 4096], [512, 512], seed=5, rows=rows, heads=[0, 3, 4, 17, 31])
    assert err <= TOL, f"max abs err {err:.2e}"


# ---- 3. past = 0 is the prefill pair ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_without_a_past_it_is_the_prefill_pair(gpu, H, Hkv, int4):
    from flash_attn.flash_attn_interface import flash_attn_varlen_func
    from qserve_amd import append as A
    r = np.random.default_rng(3 * H + Hkv)
    lens = [150, 64, 65, 1, 300]
    B, mb, W, T = len(lens), 6, (H + 2 * Hkv) * 128, sum(lens)
    tables, nblocks = scattered_tables(r, B, mb)
    src = r.standard_normal((T, W)).astype(np.float16)
    a, pools_a = dev(src), DevPools(nblocks, Hkv, int4, gpu)
    cu = _prefill_write(a, lens, pools_a.pointers(tables), H, Hkv, int4)
    q, k, v = a.split([H * 128, Hkv * 128, Hkv * 128], dim=-1)
    ref = flash_attn_varlen_func(q.reshape(T, H, 128), k.reshape(T, Hkv, 128), v.reshape(T, Hkv, 128), dev(cu), dev(cu), max(lens),
                                 max(lens), dropout_p=0.0, causal=True)
    b, pools_b = dev(src), DevPools(nblocks, Hkv, int4, gpu)
    out = A.append(b, dev(cu), dev(np.zeros(B, np.int32)), pools_b.pointers(tables), H, Hkv, _spt(Hkv, int4), BASE, int4,
                   max_seqlen_q=max(lens))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(pools_a.k, pools_b.k) and torch.equal(pools_a.v, pools_b.v)
    d = (out.float() - ref.float()).abs().max().item()
    print(f"past = 0 vs flash_attn_varlen_func: max abs diff {d:.3e}")
    assert d <= 4e-3                      # both are within 2e-3 of the same oracle


# ---- 4. n = 1 is decode -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", KV)
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_one_new_token_is_decode(gpu, H, Hkv, int4):
    from qserve_amd import append as A
    from qserve_backend import fused_attention as fa
    r = np.random.default_rng(5 * H + Hkv)
    pasts = [128, 130, 200, 1023, 640]    # contexts >= 128: none of the whitelisted short-context decode elements is involved
    B, W = len(pasts), (H + 2 * Hkv) * 128
    mb = 1024 // 64 + 1
    tables, nblocks = scattered_tables(r, B, mb)
    pools_d, pools_a = DevPools(nblocks, Hkv, int4, gpu), DevPools(nblocks, Hkv, int4, gpu)
    ctx = dev(r.standard_normal((sum(pasts), W)).astype(np.float16))
    _prefill_write(ctx.clone(), pasts, pools_d.pointers(tables), H, Hkv, int4)
    pools_a.k.copy_(pools_d.k)
    pools_a.v.copy_(pools_d.v)
    start = host_pool(_np(pools_d.k), _np(pools_d.v), Hkv, int4)
    new = r.standard_normal((B, W)).astype(np.float16)
    past, cu_q = np.asarray(pasts, np.int32), np.arange(B + 1, dtype=np.int32)

    x = dev(new)
    q, k, v = x.split([H * 128, Hkv * 128, Hkv * 128], dim=-1)
    dec = fa.single_query_attention(q.reshape(B, H, 128), k.reshape(B, Hkv, 128), v.reshape(B, Hkv, 128), pools_d.pointers(tables),
                                    dev(past + 1), None, 8192, 64, _spt(Hkv, int4), 1024, 128, BASE, True, int4, True)
    y = dev(new)
    box = _Canaried(B, H, gpu)
    A.append_rope_update_kv_cache(y, dev(cu_q), dev(past), pools_a.pointers(tables), H, Hkv, _spt(Hkv, int4), BASE, int4)
    app = A.append_attention(y, dev(cu_q), dev(past), pools_a.pointers(tables), H, Hkv, _spt(Hkv, int4), int4, max_seqlen_q=1,
                             out=box.out)
    torch.cuda.synchronize()
    box.check()
    assert torch.equal(pools_a.k, pools_d.k) and torch.equal(pools_a.v, pools_d.v), "pages after the call differ from decode's"
    # d: the distance of the two ORACLES on this case (neither side is code under test)
    o_dec = kvattn.decode_attention(new[:, : H * 128].reshape(B, H, 128), new[:, H * 128: (H + Hkv) * 128].reshape(B, Hkv, 128),
                                    new[:, (H + Hkv) * 128:].reshape(B, Hkv, 128), tables, past + 1,
                                    host_pool(start.k, start.v, Hkv, int4), BASE, mode="kernel").astype(np.float32)
    o_app = expected(rotate_rows(new, cu_q, past, H, Hkv, BASE), cu_q, past, tables, start, H, Hkv)
    d = float(np.abs(o_dec - o_app).max())
    diff = (app.float() - dec.float()).abs().max().item()
    print(f"n = 1 vs single_query_attention: max abs diff {diff:.3e}, oracle distance d {d:.3e}, "
          f"append vs its oracle {np.abs(_np(app).astype(np.float32) - o_app).max():.3e}")
    assert diff <= 1e-3 + 2e-3 + d


# ---- 6. the engine ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", [-1, 128], ids=["per_channel", "g128"])
def test_engine_prefill_chunked(gpu, gs, monkeypatch):
    from flash_attn.flash_attn_interface import flash_attn_varlen_func
    from qserve_amd import append as A
    from qserve_amd.decode import TINY, DecodeEngine
    P, CH, B = 200, 48, 3
    H, Hkv = TINY["heads"], TINY["kv_heads"]
    toks = torch.randint(0, TINY["vocab"], (B * P,), device=gpu, generator=torch.Generator(device=gpu).manual_seed(1))
    ref = DecodeEngine(TINY, batch=B, prompt_len=P, max_new=8, group_size=gs, device="cuda:0", seed=5)
    ref.prefill(P, toks)
    eng = DecodeEngine(TINY, batch=B, prompt_len=P, max_new=8, group_size=gs, device="cuda:0", seed=5)
    real, calls = A.append, []

    def checked(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, rope_theta, int4_kv, **kw):
        li, c = len(calls) % TINY["layers"], len(calls) // TINY["layers"]
        n = min(CH, P - c * CH)
        assert past_lens.tolist() == [c * CH] * B and cu_seqlens_q.tolist() == [i * n for i in range(B + 1)]
        assert kv_pointers.data_ptr() == eng.tables[li].data_ptr() and (num_heads, num_kv_heads) == (H, Hkv)
        assert qkv.shape == (B * n, eng.qkv_n) and size_per_token == eng.size_per_token and int4_kv and rope_theta == TINY["rope_theta"]
        pools_before = (eng.pools[li][0].clone(), eng.pools[li][1].clone())
        out = real(qkv, cu_seqlens_q, past_lens, kv_pointers, num_heads, num_kv_heads, size_per_token, rope_theta, int4_kv, **kw)
        # the flash emulation: de-quantised past keys uploaded as fp16, cu_q != cu_k, through the EXISTING prefill provider
        tab = ((_np(kv_pointers) - np.array([eng.pools[li][0].data_ptr(), eng.pools[li][1].data_ptr()])[None, :, None])
               // eng.page_bytes)
        hp = host_pool(_np(pools_before[0]), _np(pools_before[1]), Hkv, True)
        cu_q, past = _np(cu_seqlens_q), _np(past_lens)
        q, K, V, cu_k = compose(_np(qkv), cu_q, past, tab, hp, H, Hkv)
        emu = flash_attn_varlen_func(dev(q), dev(K), dev(V), cu_seqlens_q, dev(cu_k), n, c * CH + n, dropout_p=0.0, causal=True)
        d = (out.float() - emu.float()).abs().max().item()
        assert d <= 4e-3, f"chunk {c} layer {li}: append vs flash emulation {d:.2e}"
        calls.append(d)
        return out

    monkeypatch.setattr(A, "append", checked)
    eng.prefill_chunked(P, CH, toks)
    torch.cuda.synchronize()
    assert len(calls) == TINY["layers"] * ((P + CH - 1) // CH)
    print(f"engine gs={gs}: append vs flash emulation, max over {len(calls)} calls {max(calls):.3e}")
    # layer 0's k / v depend only on per-row-deterministic ops (embedding, norm + quant, qkv GEMM, writer)
    assert torch.equal(eng.pools[0][0], ref.pools[0][0]) and torch.equal(eng.pools[0][1], ref.pools[0][1]), "layer-0 pages differ"
    assert eng.lengths.tolist() == [P + 1] * B
    assert bool(((eng.tokens >= 0) & (eng.tokens < TINY["vocab"])).all()) and bool(torch.isfinite(eng.hidden).all())
    monkeypatch.undo()
    eng.capture()
    eng.run()
    eng.run()
    torch.cuda.synchronize()
    eng.check()
    assert eng.lengths.tolist() == [P + 4] * B        # capture() ran one warm-up step, then two replays


def test_engine_prefill_chunked_needs_less_memory(gpu):
    from qserve_amd.decode import TINY, DecodeEngine
    cfg = TINY
    peak = {}
    for name in ("whole", "chunked"):
        eng = DecodeEngine(cfg, batch=4, prompt_len=512, max_new=4, device="cuda:0", seed=2)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        eng.prefill(512) if name == "whole" else eng.prefill_chunked(512, 64)
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        del eng
    print(f"peak activation memory over the prompt: whole {peak['whole']} B, chunked {peak['chunked']} B, "
          f"ratio {peak['chunked'] / peak['whole']:.3f}")
    assert peak["chunked"] < peak["whole"]
