"""One scenario of tests/test_rope_scaling_gpu.py, as a program: `python tests/_rope_scaling_child.py <scenario>` in a FRESH process (RoPE
profiles and their tables are process-wide and never freed).  A profile's key goes wherever a rotary base goes: the prefill, append and
tree writers and single_query_attention (KV4, KV8) are compared with the numpy restatement of tests/_rope_scaling_cases.py - rotated
rows, page data bytes, fp16 scales and zeros bit for bit, attention outputs within the bar of tests/test_append_gpu.py.  Prints a
report, ends with ROPE-SCALING-OK."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np      # noqa: E402
import torch            # noqa: E402

import _rope_scaling_cases as RC                                                   # noqa: E402
import _rope_source_child as SRC                                                   # noqa: E402
from _append_cases import scattered_tables                                         # noqa: E402
from _helpers import DevPools, dev, rope_table_state                               # noqa: E402
from oracle import kvattn                                                          # noqa: E402
from qserve_amd import append as A                                                 # noqa: E402
from qserve_amd import fused, rope                                                 # noqa: E402
from qserve_amd._lib import lib                                                    # noqa: E402
from qserve_backend import fused_attention as fa                                   # noqa: E402

GPU = torch.device("cuda:0")
TOL, CFGS, PARENTS = SRC.TOL, SRC.CFGS, SRC.PARENTS
_np, _spt, _same = SRC._np, SRC._spt, SRC._same
LENS, PASTS, NS, LENGTHS = [70, 131], [0, 63, 100, 1000], [5, 3, 8, 8], [200, 64, 65, 1]


def say(*a):
    print("[rope-scaling]", *a, flush=True)


def profiles():
    return dict(llama3=rope.profile(RC.BASE, RC.LLAMA3), yarn=rope.profile(RC.BASE, RC.YARN))


# ---- the entry points under a key, each with the restatement's result computed ONCE per case -----------------------------------------
class Prefill:
    def __init__(self, prof, H, Hkv, int4, seed):
        r = np.random.default_rng(seed)
        self.H, self.Hkv, self.int4, self.mx, self.T = H, Hkv, int4, max(LENS), sum(LENS)
        self.tables, nblocks = scattered_tables(r, len(LENS), (self.mx + 63) // 64 + 1)
        self.src = r.standard_normal((self.T, (H + 2 * Hkv) * 128)).astype(np.float16)
        self.cu = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
        self.pools = DevPools(nblocks, Hkv, int4, GPU)
        self.kvp, self.d_lens = self.pools.pointers(self.tables), dev(np.asarray(LENS, np.int32))
        self.pad = fa.compute_padding_offsets(dev(self.cu), self.mx, self.T)
        if prof is not None:
            self.want = RC.expect_writer(kvattn.PagePool(nblocks, Hkv, 128, int4, fill=0xFF), self.src, self.cu, np.zeros(len(LENS), np.int32),
                                         self.tables, H, Hkv, prof)

    def call(self, key, rows):
        fa.apply_bias_rope_update_kv_cache(rows, self.d_lens, self.pad, self.kvp, self.H, self.Hkv, self.mx, 64, _spt(self.Hkv, self.int4), 128, key,
                                           8192, True, self.int4, True)

    def run(self, key, what, check=True):
        self.pools.k.fill_(0xFF), self.pools.v.fill_(0xFF)
        rows = dev(self.src)
        self.call(key, rows)
        torch.cuda.synchronize()
        got = (_np(rows), _np(self.pools.k), _np(self.pools.v))
        if check:
            _same(got, self.want, f"prefill writer {what} H={self.H} Hkv={self.Hkv} int4={self.int4}")
        return got


class Append(SRC.Append):
    """_rope_source_child.Append with the history and the expected values of a PROFILE (base = the key at call time)."""

    def __init__(self, prof, H, Hkv, int4, pasts, ns, mb, seed, history=True):
        super().__init__(RC.BASE, H, Hkv, int4, pasts, ns, mb, seed, history=False)
        self.prof = prof
        if history and prof is not None:
            RC.history(self.host0, np.random.default_rng(seed + 1000), self.tables, pasts, H, Hkv, prof)
            self.reset()

    def expect_writer(self, tree):
        return RC.expect_writer(self.host0, self.src, self.cu_q, self.past, self.tables, self.H, self.Hkv, self.prof, self.words if tree else None)

    def run(self, key, tree, what, check=True):
        self.base = key
        self.reset()
        rows = dev(self.src)
        self.write(rows, tree)
        torch.cuda.synchronize()
        got = (_np(rows), _np(self.pools.k), _np(self.pools.v))
        if check:
            _same(got, self.expect_writer(tree), f"{'tree' if tree else 'append'} writer {what} H={self.H} Hkv={self.Hkv} int4={self.int4}")
        return got


class Decode:
    def __init__(self, prof, H, Hkv, int4, lengths, seed):
        r = np.random.default_rng(seed)
        self.H, self.Hkv, self.int4, self.B = H, Hkv, int4, len(lengths)
        self.lengths = np.asarray(lengths, np.int32)
        self.tables, nblocks = scattered_tables(r, self.B, (max(lengths) + 63) // 64 + 1)
        self.host0 = kvattn.PagePool(nblocks, Hkv, 128, int4, fill=0xFF)
        RC.history(self.host0, r, self.tables, [L - 1 for L in lengths], H, Hkv, prof)
        self.new = r.standard_normal((self.B, (H + 2 * Hkv) * 128)).astype(np.float16)
        self.ref, self.want_k, self.want_v = RC.expect_decode(self.host0, self.new, self.lengths, self.tables, H, Hkv, prof)
        self.pools = DevPools(nblocks, Hkv, int4, GPU)
        self.kvp, self.d_new, self.d_len = self.pools.pointers(self.tables), dev(self.new), dev(self.lengths)

    def reset(self):
        self.pools.k.copy_(dev(self.host0.k))
        self.pools.v.copy_(dev(self.host0.v))

    def qkv(self):
        return [x.reshape(self.B, -1, 128) for x in self.d_new.split([self.H * 128, self.Hkv * 128, self.Hkv * 128], dim=-1)]

    def call(self, key, max_seqlen):
        q, k, v = self.qkv()
        return fa.single_query_attention(q, k, v, self.kvp, self.d_len, None, max_seqlen, 64, _spt(self.Hkv, self.int4), int(self.lengths.max()), 128,
                                         key, True, self.int4, True)

    def check(self, got, what):
        what = f"decode {what} H={self.H} Hkv={self.Hkv} int4={self.int4}"
        for x, y, n_ in zip(got[1:], (self.want_k, self.want_v), ("K pages", "V pages")):
            assert np.array_equal(x, y), f"{what}: {n_} differ"
        err = float(np.abs(got[0].astype(np.float32) - self.ref).max())
        assert np.isfinite(got[0].astype(np.float32)).all() and err <= TOL, f"{what}: max abs err {err:.2e}"
        return got

    def run(self, key, max_seqlen, what):
        self.reset()
        out = self.call(key, max_seqlen)
        torch.cuda.synchronize()
        return self.check((_np(out), _np(self.pools.k), _np(self.pools.v)), what)


def _state(key):
    return rope.profile_state(key)


def _register_raw(denom, mscale, rows):
    key = ctypes.c_float(0.0)
    d = np.ascontiguousarray(denom, np.float32)
    rc = lib.qs_rope_profile_register(d.ctypes.data_as(ctypes.c_void_p), 64, float(mscale), rows, ctypes.byref(key))
    return rc, key.value, (lib.qs_last_error() or b"").decode()


# ---- scenarios ------------------------------------------------------------------------------------------------------------------------
def table():
    """Both profiles registered with 2048 positions; the five entry points against the restatement, every row from the table.  Then the
    forms that carry no table of their own, once: the VALU decode kernel and the per-lane prefill writer (qs_set_attention_variant), and
    the attention + quant fusion against the un-fused pair."""
    for pi, (name, prof) in enumerate(profiles().items()):
        assert prof[1] == 1.0 if name == "llama3" else prof[1] != 1.0
        key = rope.register(prof[0], prof[1], 2048)
        assert key == -(pi + 1) and _state(key) == (pi + 1, 2048), (key, _state(key))
        for i, (H, Hkv, int4) in enumerate(CFGS):
            p = Prefill(prof, H, Hkv, int4, 10 + i)
            p.run(key, name)
            a = Append(prof, H, Hkv, int4, PASTS, NS, 17, 20 + i)
            w = a.run(key, False, name)
            a.run(key, True, name)
            a.reset()
            err = a.check_attention(w[0], _np(a.attend(dev(w[0]))), f"append attention {name}")
            d = Decode(prof, H, Hkv, int4, LENGTHS, 30 + i)
            d.run(key, 2048, name)
            assert _state(key) == (pi + 1, 2048), "every row was covered: no longer table"
            lib.qs_set_attention_variant(1)
            d.run(key, 2048, f"{name} VALU kernel")
            lib.qs_set_attention_variant(2)
            p.run(key, f"{name} per-lane form")
            a.run(key, False, f"{name} table-less form")
            lib.qs_set_attention_variant(0)
            say(f"{name} key {key:g} H={H} Hkv={Hkv} int4={int4}: prefill, append, tree, decode (+ VALU, per-lane) match; append attention err {err:.2e}")
        # the fusion (KV4, un-split): bit-equal to attention followed by invoke_quant
        H, Hkv = CFGS[0][:2]
        d = Decode(prof, H, Hkv, True, LENGTHS, 39)
        plain = d.run(key, 2048, f"{name} un-fused")
        d.reset()
        qo = torch.empty((d.B, H * 128), dtype=torch.int8, device=GPU)
        qs, qsum = torch.empty((d.B,), dtype=torch.float16, device=GPU), torch.empty((d.B,), dtype=torch.float16, device=GPU)
        q, k, v = d.qkv()
        out = fused.single_query_attention_quant(q, k, v, d.kvp, d.d_len, qo, qs, 2048, 64, _spt(Hkv, True), int(d.lengths.max()), 128, key, True,
                                                 True, True, quant_sum=qsum)
        torch.cuda.synchronize()
        _same(d.check((_np(out), _np(d.pools.k), _np(d.pools.v)), f"{name} attention + quant"), plain, f"{name}: fused against un-fused")
        assert np.isfinite(_np(qs).astype(np.float32)).all()
    # an eager call that needs more rows builds a longer table for the key; the old one stays
    key = -1.0
    Decode(profiles()["llama3"], *CFGS[0], [2100], 38).run(key, 4096, "llama3 longer table")
    assert _state(key) == (2, 4096), _state(key)


def beyond():
    """A 64-row table, and the calls captured so that no longer one can be built: one decode launch holds positions 0 and 63 (table) and
    64 and 199 (in the kernel), the prefill writer runs per lane, the append and tree writers have rows at 1000.  Bytes equal to the
    restatement, and to the same calls made eagerly afterwards, which build a table that covers everything."""
    for pi, (name, prof) in enumerate(profiles().items()):
        H0, Hkv0, k40 = CFGS[0]
        # (the device code of every entry is loaded by eager calls on a PLAIN base before anything is captured)
        if pi == 0:
            SRC.prefill(5e5, H0, Hkv0, k40, [70], 58)
            w = SRC.Append(5e5, H0, Hkv0, k40, [100], [5], 3, 59)
            w.writer(), w.writer(tree=True)
            for k4 in (True, False):
                SRC.Decode(5e5, H0, Hkv0, k4, [70], 59).run(64)
        key = rope.register(prof[0], prof[1], 64)
        assert _state(key) == (pi + 1, 64)
        caps = []
        for i, (H, Hkv, int4) in enumerate(CFGS):
            p = Prefill(prof, H, Hkv, int4, 40 + i)
            a = Append(prof, H, Hkv, int4, PASTS, NS, 17, 44 + i, history=False)
            d = Decode(prof, H, Hkv, int4, LENGTHS, 48 + i)
            a.base = key
            a.reset(), d.reset()
            p.pools.k.fill_(0xFF), p.pools.v.fill_(0xFF)
            srcs = [dev(p.src), dev(a.src), dev(a.src)]
            rows = [torch.empty_like(s) for s in srcs]
            tree_pools = DevPools(a.nblocks, Hkv, int4, GPU)
            tree_kvp = tree_pools.pointers(a.tables)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for r_, s_ in zip(rows, srcs):
                    r_.copy_(s_)
                p.call(key, rows[0])
                a.write(rows[1])
                A.append_tree_rope_update_kv_cache(rows[2], a.d_cu, a.d_past, tree_kvp, a.d_words, H, Hkv, _spt(Hkv, int4), key, int4)
                out = d.call(key, 8192)
            assert _state(key) == (pi + 1, 64), "a capture must not build a table"
            g.replay()
            torch.cuda.synchronize()
            assert _state(key) == (pi + 1, 64)
            cap = [(_np(rows[0]), _np(p.pools.k), _np(p.pools.v)), (_np(rows[1]), _np(a.pools.k), _np(a.pools.v)),
                   (_np(rows[2]), _np(tree_pools.k), _np(tree_pools.v)), (_np(out), _np(d.pools.k), _np(d.pools.v))]
            what = f"{name} 64-row table, captured, H={H} Hkv={Hkv} int4={int4}"
            _same(cap[0], p.want, f"prefill writer {what}")
            _same(cap[1], a.expect_writer(False), f"append writer {what}")
            _same(cap[2], a.expect_writer(True), f"tree writer {what}")
            d.check(cap[3], what)
            caps.append((p, a, d, cap, what))
            say(f"{what}: rows at 64, 199 (decode), 64 .. 130 (prefill), 1000 .. (writers) evaluated in the kernel: restatement's bytes")
        # now eagerly: the decode call asks for 8192 rows and gets them, every later call reads that table
        for i, (p, a, d, cap, what) in enumerate(caps):
            if i == 0:
                d.run(key, 8192, name)
                assert _state(key) == (pi + 1, 8192), _state(key)
            full = [p.run(key, name), a.run(key, False, name), a.run(key, True, name), d.run(key, 8192, name)]
            assert _state(key) == (pi + 1, 8192), _state(key)
            for c_, f_, n_ in zip(cap, full, ("prefill", "append", "tree", "decode")):
                _same(c_, f_, f"{n_} {what}: in-kernel rows against the 8192-row table")
        say(f"{name}: the same calls with an 8192-row table: the captured bytes")


def capture():
    """Writers and decode captured AFTER registration with a covering table, replayed twice: the same bytes each time, equal to eager."""
    name, prof = "yarn", profiles()["yarn"]
    key = rope.register(prof[0], prof[1], 2048)
    with_capture, scratch = None, torch.zeros(8, device=GPU)
    torch.cuda.synchronize()
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
        scratch.add_(1.0)
        try:
            rope.register(profiles()["llama3"][0], 1.0, 2048)
        except RuntimeError as e:
            with_capture = str(e)
    assert with_capture and "stream capture" in with_capture, with_capture
    assert _state(key)[0] == 1, "a registration inside a capture registers nothing"
    for i, (H, Hkv, int4) in enumerate(CFGS):
        p = Prefill(prof, H, Hkv, int4, 60 + i)
        a = Append(prof, H, Hkv, int4, PASTS, NS, 17, 64 + i)
        d = Decode(prof, H, Hkv, int4, LENGTHS, 68 + i)
        eager = [p.run(key, name), a.run(key, False, name), d.run(key, 2048, name)]
        srcs = [dev(p.src), dev(a.src)]
        rows = [torch.empty_like(s) for s in srcs]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for r_, s_ in zip(rows, srcs):
                r_.copy_(s_)
            p.call(key, rows[0])
            a.write(rows[1])
            out = d.call(key, 2048)
        for rep in range(2):
            p.pools.k.fill_(0xFF), p.pools.v.fill_(0xFF)
            a.reset(), d.reset()
            g.replay()
            torch.cuda.synchronize()
            got = [(_np(rows[0]), _np(p.pools.k), _np(p.pools.v)), (_np(rows[1]), _np(a.pools.k), _np(a.pools.v)),
                   (_np(out), _np(d.pools.k), _np(d.pools.v))]
            for g_, e_, n_ in zip(got, eager, ("prefill", "append", "decode")):
                _same(g_, e_, f"replay {rep}: captured {n_} against eager, H={H} Hkv={Hkv} int4={int4}")
        assert _state(key) == (1, 2048)
        say(f"{name} H={H} Hkv={Hkv} int4={int4}: captured prefill, append writer and decode, two replays: the eager bytes")


def plain():
    """Two profiles registered; a plain base 1e6 then runs the five entries to the ORACLE's bytes and its table slots are what they are
    without profiles; profile and plain results differ; ids are content-addressed; the ninth profile and unknown keys are errors."""
    base = 1e6
    profs = profiles()
    keys = [rope.register(p[0], p[1], 2048) for p in profs.values()]
    assert keys == [-1.0, -2.0] and rope.register(profs["llama3"][0], profs["llama3"][1], 64) == -1.0
    assert _state(-1.0) == (2, 2048) and _state(-2.0) == (2, 2048) and _state(-3.0) == (2, 0) and _state(1e6) == (2, 0)
    assert rope_table_state(base) == (0, 0), "profile tables live beside the base slots"
    H, Hkv, int4 = CFGS[0]
    SRC.prefill(base, H, Hkv, int4, LENS, 80)
    assert rope_table_state(base) == (1, 131)
    a = SRC.Append(base, H, Hkv, int4, PASTS, NS, 17, 81, history=False)
    wp = a.writer()
    assert rope_table_state(base) == (2, 2048)
    tp = a.writer(tree=True)
    dp = [SRC.Decode(base, H, Hkv, k4, LENGTHS, 82).run(8192) for k4 in (True, False)]
    assert rope_table_state(base) == (3, 8192), rope_table_state(base)      # what tests/_rope_source_child.py `fresh` pins without profiles
    assert _state(-1.0) == (2, 2048)
    # the same inputs under a profile: other bytes
    b = Append(profs["llama3"], H, Hkv, int4, PASTS, NS, 17, 81, history=False)
    assert np.array_equal(b.src, a.src)
    wk, tk = b.run(-1.0, False, "llama3"), b.run(-1.0, True, "llama3")
    assert not np.array_equal(wk[0], wp[0]) and not np.array_equal(wk[1], wp[1]) and not np.array_equal(tk[0], tp[0])
    wy = Append(profs["yarn"], H, Hkv, int4, PASTS, NS, 17, 81, history=False).run(-2.0, False, "yarn")
    assert not np.array_equal(wy[0], wk[0])
    say("plain base 1e6 with two profiles registered: oracle bytes, table slots (3, 8192); profile runs differ")
    # errors: nothing is launched (the buffers keep their bytes)
    for bad in (-3.0, -9.0, -1.5, -1e30):
        rows = dev(a.src)
        b.pools.k.fill_(0x5A)
        b.base = bad
        for tree in (False, True):
            try:
                b.write(rows, tree)
                raise AssertionError(f"key {bad}: the writer accepted an unregistered key")
            except RuntimeError as e:
                assert "code -1" in str(e) and "profile" in str(e), str(e)
        p = Prefill(None, H, Hkv, int4, 83)
        prow = dev(p.src)
        d = Decode(profs["llama3"], H, Hkv, int4, [5], 84)
        d.reset()
        for fn in (lambda: p.call(bad, prow), lambda: d.call(bad, 64)):
            try:
                fn()
                raise AssertionError(f"key {bad}: an entry accepted an unregistered key")
            except RuntimeError as e:
                assert "profile" in str(e), str(e)
        torch.cuda.synchronize()
        assert np.array_equal(_np(rows), a.src) and np.array_equal(_np(prow), p.src) and bool((b.pools.k == 0x5A).all())
        assert np.array_equal(_np(d.pools.k), d.host0.k) and bool((p.pools.k == 0xFF).all())
    for i in range(6):
        rc, key, msg = _register_raw(profs["llama3"][0] * np.float32(2 + i), 1.0, 64)
        assert (rc, key) == (0, -(3.0 + i)), (rc, key, msg)
    rc, key, msg = _register_raw(profs["llama3"][0] * np.float32(9), 1.0, 64)
    assert rc == -1 and "8 RoPE profiles" in msg and _state(-9.0) == (8, 0), (rc, msg)
    assert _register_raw(profs["yarn"][0], profs["yarn"][1], 64)[:2] == (0, -2.0), "a registered profile still resolves with all ids taken"
    d32 = np.ascontiguousarray(profs["yarn"][0], np.float32)
    key_c = ctypes.c_float(0.0)
    assert lib.qs_rope_profile_register(d32.ctypes.data_as(ctypes.c_void_p), 32, 1.0, 64, ctypes.byref(key_c)) == -1 and b"pairs=32" in lib.qs_last_error()
    assert lib.qs_rope_profile_register(d32.ctypes.data_as(ctypes.c_void_p), 64, 1.0, 40000, ctypes.byref(key_c)) == -1
    assert rope_table_state(base) == (3, 8192)
    _same(a.writer(), wp, "plain base after everything")
    say("same profile twice: one key; ninth profile, unregistered and malformed keys: QS_EINVAL with a message, nothing launched")


SCENARIOS = dict(table=table, beyond=beyond, capture=capture, plain=plain)

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]]()
    torch.cuda.synchronize()
    print("ROPE-SCALING-OK", sys.argv[1], flush=True)
