"""One scenario of tests/test_rope_source_gpu.py, as a program: `python tests/_rope_source_child.py <scenario>` in a FRESH process (the
library's RoPE tables are process-wide and never freed).  Where the cos / sin values of a call come from - a table, or the in-kernel
evaluation - is read from qs_debug_rope_table_state before and after the call and asserted; every writer result (rotated rows, page
data bytes, fp16 scale, fp16 zero) is compared with the numpy oracle bit for bit, every attention output bit for bit between the two
sources of one base (and with the float64 oracle at the bar of the fp16 attention tests).  Prints a report, ends with ROPE-SOURCE-OK."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np      # noqa: E402
import torch            # noqa: E402

from _append_cases import expected, host_pool, rotate_rows, scattered_tables      # noqa: E402
from _helpers import DevPools, dev, rope_table_state as state                      # noqa: E402
from _tree_cases import as_int64, rotate_rows_tree, words_from_parents             # noqa: E402
from oracle import kvattn                                                          # noqa: E402
from qserve_amd import append as A                                                 # noqa: E402
from qserve_backend import fused_attention as fa                                   # noqa: E402

GPU = torch.device("cuda:0")
TOL = 2e-3      # tests/test_append_gpu.py
CFGS = [(8, 2, True), (8, 2, False), (4, 4, True), (4, 4, False)]
PARENTS = [-1, 0, 0, 1, 3, -1, 5, 5]      # depths 0 1 1 2 3 0 1 1 (cut to a sequence's n)


def say(*a):
    print("[rope-source]", *a, flush=True)


def _np(t):
    return t.detach().cpu().numpy()


def _spt(Hkv, int4):
    return Hkv * (64 if int4 else 128)


def _same(a, b, what):
    for x, y, name in zip(a, b, ("rows / out", "K pages", "V pages", "extra")):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), f"{what}: {name} differ"


# ---- the five entry points, each against the oracle ---------------------------------------------------------------------------------
def prefill(base, H, Hkv, int4, lens, seed):
    """The prefill writer on fresh 0xFF pools -> (rows, K pool, V pool), bit-equal to kvattn.prefill_update_kv_cache."""
    r = np.random.default_rng(seed)
    B, T, mx = len(lens), sum(lens), max(lens)
    tables, nblocks = scattered_tables(r, B, (mx + 63) // 64 + 1)
    src = r.standard_normal((T, (H + 2 * Hkv) * 128)).astype(np.float16)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    pools = DevPools(nblocks, Hkv, int4, GPU)
    rows = dev(src)
    fa.apply_bias_rope_update_kv_cache(rows, dev(np.asarray(lens, np.int32)), fa.compute_padding_offsets(dev(cu), mx, T), pools.pointers(tables),
                                       H, Hkv, mx, 64, _spt(Hkv, int4), 128, base, 8192, True, int4, True)
    torch.cuda.synchronize()
    want = kvattn.PagePool(nblocks, Hkv, 128, int4, fill=0xFF)
    wrows = src.copy()
    kvattn.prefill_update_kv_cache(wrows, np.asarray(lens, np.int32), kvattn.compute_padding_offsets(cu, mx, T), tables, want, H, Hkv, mx, base)
    got = (_np(rows), _np(pools.k), _np(pools.v))
    _same(got, (wrows, want.k, want.v), f"prefill writer base {base:g} H={H} Hkv={Hkv} int4={int4}")
    return got


class Append:
    """pasts / ns on scattered tables of mb entries; the pages below `past` hold a history written by the ORACLE on the host (no device
    call, so no table is asked for), every other byte is 0xFF."""

    def __init__(self, base, H, Hkv, int4, pasts, ns, mb, seed, history=True):
        r = np.random.default_rng(seed)
        self.base, self.H, self.Hkv, self.int4, self.mb = base, H, Hkv, int4, mb
        self.B, self.W = len(pasts), (H + 2 * Hkv) * 128
        self.tables, self.nblocks = scattered_tables(r, self.B, mb)
        self.host0 = kvattn.PagePool(self.nblocks, Hkv, 128, int4, fill=0xFF)
        if history:
            for b, p in enumerate(pasts):
                if p:
                    ctx = r.standard_normal((p, self.W)).astype(np.float16)
                    kvattn.prefill_update_kv_cache(ctx, np.asarray([p], np.int32), np.zeros(p, np.int32), self.tables[b:b + 1], self.host0, H, Hkv, p, base)
        self.cu_q = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
        self.past = np.asarray(pasts, np.int32)
        self.T = int(self.cu_q[-1])
        self.src = r.standard_normal((self.T, self.W)).astype(np.float16)
        self.words = [w for n in ns for w in words_from_parents(PARENTS[:n])]
        self.pools = DevPools(self.nblocks, Hkv, int4, GPU)
        self.kvp = self.pools.pointers(self.tables)
        self.d_cu, self.d_past, self.d_words = dev(self.cu_q), dev(self.past), dev(as_int64(self.words))
        self.msq = int(max(ns))
        self.reset()

    def reset(self):
        self.pools.k.copy_(dev(self.host0.k))
        self.pools.v.copy_(dev(self.host0.v))

    def expect_writer(self, tree):
        """-> (rotated rows, K pool, V pool) of the oracle: rotated at past + i (tree: past + depth), stored at past + i."""
        H, Hkv = self.H, self.Hkv
        rot = (rotate_rows_tree(self.src, self.cu_q, self.past, self.words, H, Hkv, self.base) if tree else
               rotate_rows(self.src, self.cu_q, self.past, H, Hkv, self.base))
        want = host_pool(self.host0.k, self.host0.v, Hkv, self.int4)
        kb, ks, kz = kvattn.kv_quantize(rot[:, H * 128:(H + Hkv) * 128].reshape(-1, Hkv, 128), self.int4)
        vb, vs, vz = kvattn.kv_quantize(self.src[:, (H + Hkv) * 128:].reshape(-1, Hkv, 128), self.int4)
        for b in range(self.B):
            for i, t in enumerate(range(int(self.cu_q[b]), int(self.cu_q[b + 1]))):
                pos = int(self.past[b]) + i
                for h in range(Hkv):
                    want.write_token("k", int(self.tables[b, 0, pos // 64]), pos % 64, h, kb[t, h], ks[t, h], kz[t, h])
                    want.write_token("v", int(self.tables[b, 1, pos // 64]), pos % 64, h, vb[t, h], vs[t, h], vz[t, h])
        return rot, want.k, want.v

    def write(self, rows, tree=False):
        if tree:
            A.append_tree_rope_update_kv_cache(rows, self.d_cu, self.d_past, self.kvp, self.d_words, self.H, self.Hkv, _spt(self.Hkv, self.int4),
                                               self.base, self.int4)
        else:
            A.append_rope_update_kv_cache(rows, self.d_cu, self.d_past, self.kvp, self.H, self.Hkv, _spt(self.Hkv, self.int4), self.base, self.int4)

    def attend(self, rows, out=None):
        return A.append_attention(rows, self.d_cu, self.d_past, self.kvp, self.H, self.Hkv, _spt(self.Hkv, self.int4), self.int4,
                                  max_seqlen_q=self.msq, out=out)

    def writer(self, tree=False):
        """One writer launch on fresh pages -> (rows, K pool, V pool), bit-equal to the oracle."""
        self.reset()
        rows = dev(self.src)
        self.write(rows, tree)
        torch.cuda.synchronize()
        got = (_np(rows), _np(self.pools.k), _np(self.pools.v))
        _same(got, self.expect_writer(tree), f"{'tree' if tree else 'append'} writer base {self.base:g} H={self.H} Hkv={self.Hkv} int4={self.int4}")
        return got

    def check_attention(self, rows, out, what):
        ref = expected(rows, self.cu_q, self.past, self.tables, self.host0, self.H, self.Hkv)
        err = float(np.abs(out.astype(np.float32) - ref).max())
        assert np.isfinite(out.astype(np.float32)).all() and err <= TOL, f"{what}: max abs err {err:.2e}"
        return err


class Decode:
    """single_query_attention at `lengths` (the new token included) over a history the ORACLE wrote on the host."""

    def __init__(self, base, H, Hkv, int4, lengths, seed):
        r = np.random.default_rng(seed)
        self.base, self.H, self.Hkv, self.int4 = base, H, Hkv, int4
        self.B, W = len(lengths), (H + 2 * Hkv) * 128
        self.lengths = np.asarray(lengths, np.int32)
        self.mb = (max(lengths) + 63) // 64 + 1
        self.tables, self.nblocks = scattered_tables(r, self.B, self.mb)
        self.host0 = kvattn.PagePool(self.nblocks, Hkv, 128, int4, fill=0xFF)
        for b, L in enumerate(lengths):
            if L > 1:
                ctx = r.standard_normal((L - 1, W)).astype(np.float16)
                kvattn.prefill_update_kv_cache(ctx, np.asarray([L - 1], np.int32), np.zeros(L - 1, np.int32), self.tables[b:b + 1], self.host0, H, Hkv,
                                               L - 1, base)
        self.new = r.standard_normal((self.B, W)).astype(np.float16)
        q, k, v = np.split(self.new, [H * 128, (H + Hkv) * 128], axis=1)
        want = host_pool(self.host0.k, self.host0.v, Hkv, int4)
        self.ref = kvattn.decode_attention(q.reshape(self.B, H, 128), k.reshape(self.B, Hkv, 128), v.reshape(self.B, Hkv, 128), self.tables,
                                           self.lengths, want, base, "exact").astype(np.float32)
        self.want = want            # (decode_attention wrote the new token's slots)
        self.pools = DevPools(self.nblocks, Hkv, int4, GPU)
        self.kvp = self.pools.pointers(self.tables)
        self.d_new, self.d_len = dev(self.new), dev(self.lengths)

    def reset(self):
        self.pools.k.copy_(dev(self.host0.k))
        self.pools.v.copy_(dev(self.host0.v))

    def call(self, max_seqlen):
        H, Hkv, B = self.H, self.Hkv, self.B
        q, k, v = [x.reshape(B, -1, 128) for x in self.d_new.split([H * 128, Hkv * 128, Hkv * 128], dim=-1)]
        return fa.single_query_attention(q, k, v, self.kvp, self.d_len, None, max_seqlen, 64, _spt(Hkv, self.int4), int(self.lengths.max()), 128,
                                         self.base, True, self.int4, True)

    def run(self, max_seqlen):
        """-> (out, K pool, V pool): the pages bit-equal to the oracle's, the output within TOL of the float64 attention."""
        self.reset()
        out = self.call(max_seqlen)
        torch.cuda.synchronize()
        return self.check((_np(out), _np(self.pools.k), _np(self.pools.v)), f"max_seqlen {max_seqlen}")

    def check(self, got, what):
        what = f"decode base {self.base:g} H={self.H} Hkv={self.Hkv} int4={self.int4} {what}"
        _same(got[1:], (self.want.k, self.want.v), what)
        err = float(np.abs(got[0].astype(np.float32) - self.ref).max())
        assert np.isfinite(got[0].astype(np.float32)).all() and err <= TOL, f"{what}: max abs err {err:.2e}"
        return got


# ---- scenarios ------------------------------------------------------------------------------------------------------------------------
def fresh():
    """Nothing exists; the five entry points on base 1e6, eagerly: each gets a table that covers what it asked for."""
    base = 1e6
    assert state(base) == (0, 0), state(base)
    for i, (H, Hkv, int4) in enumerate(CFGS):
        prefill(base, H, Hkv, int4, [70, 131], 10 + i)
        s = state(base)
        say(f"prefill writer H={H} Hkv={Hkv} int4={int4}: tables (slots, rows for 1e6) {s}")
        assert s[1] >= 131 and s[0] >= 1
        if i == 0:
            assert s == (1, 131), s
        a = Append(base, H, Hkv, int4, [0, 63, 100, 1000], [5, 3, 8, 8], 17, 20 + i, history=False)
        a.writer()
        s = state(base)
        assert s[1] >= 2048 and (i > 0 or s == (2, 2048)), s
        a.writer(tree=True)
        assert state(base) == s, "the tree writer shares the append writer's table"
        say(f"append + tree writers H={H} Hkv={Hkv} int4={int4}: tables {s}")
        d = Decode(base, H, Hkv, int4, [200, 64, 65, 1], 30 + i)
        d.run(8192)
        s = state(base)
        assert s[1] >= 8192 and (i > 0 or s == (3, 8192)), s
        say(f"decode H={H} Hkv={Hkv} int4={int4}: tables {s}")
    assert state(base) == (3, 8192)


def short_table():
    """A 64-row table and tl = 199, 63, 64, 0 in one launch (table rows 63 and 0, in-kernel 199 and 64), then the same call with a
    table that covers everything: outputs and pages bit-equal.  One base per configuration: each starts without a table."""
    for i, ((H, Hkv, int4), base) in enumerate(zip(CFGS, [1e6, 5e5, 1e4, 2e5])):
        d = Decode(base, H, Hkv, int4, [200, 64, 65, 1], 40 + i)
        assert state(base) == (2 * i, 0), state(base)
        mixed = d.run(64)
        assert state(base) == (2 * i + 1, 64), state(base)
        full = d.run(8192)
        assert state(base) == (2 * i + 2, 8192), state(base)
        _same(mixed, full, f"decode H={H} Hkv={Hkv} int4={int4}: 64-row table + in-kernel against the 8192-row table")
        say(f"decode H={H} Hkv={Hkv} int4={int4} base {base:g}: 64-row table (positions 64 and 199 in the kernel) == 8192-row table, bit for bit")


def boundary_writers():
    """The append and tree writers with a pointer table beyond 32 768 tokens get the clamped 32 768-row table: one launch with rows at
    32 766 .. 32 770 (both sides of the last table row), a sequence wholly below and one wholly above."""
    base = 1e6
    assert state(base) == (0, 0)
    for i, (H, Hkv, int4) in enumerate(CFGS):
        a = Append(base, H, Hkv, int4, [32766, 100, 40000], [5, 8, 5], 640, 50 + i, history=False)
        a.writer()
        assert state(base) == (1, 32768), state(base)
        a.writer(tree=True)
        assert state(base) == (1, 32768), state(base)
        say(f"append + tree writers H={H} Hkv={Hkv} int4={int4}: rows 32766 .. 32770, 100 .., 40000 .. with the 32768-row table: oracle bytes")


def capture():
    """The first calls of the process on a base arrive inside a stream capture: no table can be built, the graph holds the in-kernel
    evaluation.  Replays against the oracle, then the same calls eagerly (a table now exists): equal bytes."""
    base, (H, Hkv, int4) = 1e6, CFGS[0]
    # (the same entry points once on ANOTHER base, eagerly: the library's device code is loaded before the capture begins)
    w = Append(5e5, H, Hkv, int4, [100], [5], 3, 59)
    w.attend(dev(w.writer()[0]))
    for k4 in (True, False):
        Decode(5e5, H, Hkv, k4, [70], 59).run(64)
    slots0 = state(base)
    assert slots0[1] == 0, slots0
    a = Append(base, H, Hkv, int4, [100, 63, 2040], [5, 8, 8], 34, 60)
    ds = [Decode(base, H, Hkv, k4, [200, 64, 65, 1], 61 + int(k4)) for k4 in (True, False)]
    for d in ds:
        d.reset()
    src = dev(a.src)
    rows = torch.empty_like(src)
    out = torch.zeros((a.T, H, 128), dtype=torch.float16, device=GPU)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rows.copy_(src)
        a.write(rows)
        a.attend(rows, out=out)
        douts = [d.call(8192) for d in ds]
    assert state(base) == slots0, f"a capture must not build a table: {state(base)}"
    want = a.expect_writer(False)
    replayed = None
    for rep in range(2):
        a.reset()
        for d in ds:
            d.reset()
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert state(base) == slots0
        got = (_np(rows), _np(a.pools.k), _np(a.pools.v), _np(out))
        _same(got[:3], want, f"replay {rep}: captured append writer (in-kernel)")
        err = a.check_attention(got[0], got[3], f"replay {rep}: captured append attention")
        dgot = [d.check((_np(o), _np(d.pools.k), _np(d.pools.v)), f"replay {rep} (in-kernel)") for d, o in zip(ds, douts)]
        if replayed is not None:
            _same(got, replayed[0], "replay 1 against replay 0")
        replayed = (got, dgot)
    say(f"captured first calls: no table for 1e6 after capture and two replays; append attention max abs err {err:.2e}")
    a.reset()
    erows = dev(a.src)
    a.write(erows)
    eout = a.attend(erows)
    torch.cuda.synchronize()
    s1 = state(base)
    assert s1 == (slots0[0] + 1, 4096), s1      # the append writer asks for the table's reach (34 pages) rounded up to a power of two
    _same((_np(erows), _np(a.pools.k), _np(a.pools.v), _np(eout)), replayed[0], "eager (table) against the replayed graph (in-kernel)")
    for d, rg in zip(ds, replayed[1]):
        _same(d.run(8192), rg, f"decode int4={d.int4}: eager (table) against the replayed graph (in-kernel)")
    assert state(base) == (slots0[0] + 2, 8192), state(base)
    say(f"eager calls afterwards: tables {s1} then {state(base)}; bytes equal to the replays")


def exhausted():
    """Eight bases take the eight slots; a ninth gets no table, ever: the five entry points evaluate in the kernel."""
    H, Hkv, int4 = CFGS[0]
    bases = [1e4 * (i + 1) for i in range(8)]
    first = []
    for i, b in enumerate(bases):
        first.append(prefill(b, H, Hkv, int4, [5], 70))
        assert state(b) == (i + 1, 5), state(b)
    ninth = 5e5
    assert state(ninth) == (8, 0)
    for i, (H, Hkv, int4) in enumerate(CFGS):
        prefill(ninth, H, Hkv, int4, [70, 131], 71 + i)
        a = Append(ninth, H, Hkv, int4, [0, 63, 100, 2046], [5, 3, 8, 5], 34, 75 + i, history=False)
        a.writer()
        a.writer(tree=True)
        Decode(ninth, H, Hkv, int4, [200, 64, 65, 1], 80 + i).run(8192)
        assert state(ninth) == (8, 0), state(ninth)
    say("ninth base 5e5 with 8 slots taken: prefill, append, tree writers and decode (KV4, KV8) match the oracle, no table")
    H, Hkv, int4 = CFGS[0]
    for i in (0, 3, 7):
        _same(prefill(bases[i], H, Hkv, int4, [5], 70), first[i], f"base {bases[i]:g} again")
        assert state(bases[i]) == (8, 5)
    say("bases 1, 4 and 8 of the eight resolve to their own tables: results equal to their first runs")


def interleaved():
    """Base A, base B, base A on the same buffers: the third result is the first, A's differs from B's."""
    H, Hkv, int4 = CFGS[0]
    res = []
    for base in (1e4, 1e6, 1e4):
        a = Append(base, H, Hkv, int4, [100, 63, 1000], [5, 8, 8], 17, 90)
        w = a.writer()
        t = a.writer(tree=True)
        rows = dev(w[0])
        a.reset()
        out = _np(a.attend(rows))
        a.check_attention(w[0], out, f"append attention base {base:g}")
        dd = [Decode(base, H, Hkv, k4, [200, 64, 65, 1], 91).run(8192) for k4 in (True, False)]
        res.append((w, t, (out,), dd[0], dd[1]))
        say(f"base {base:g}: tables {state(base)}")
    assert state(1e4) == (4, 8192) and state(1e6) == (4, 8192), (state(1e4), state(1e6))
    for x, y, z, name in zip(res[0], res[1], res[2], ("append writer", "tree writer", "append attention", "decode KV4", "decode KV8")):
        _same(x, z, f"{name}: base 1e4 after base 1e6 against base 1e4 before")
        assert not np.array_equal(x[0], y[0]), f"{name}: base 1e4 and base 1e6 give the same result"
    say("1e4, 1e6, 1e4: the third result equals the first bit for bit, and differs from the second")


SCENARIOS = dict(fresh=fresh, short_table=short_table, boundary_writers=boundary_writers, capture=capture, exhausted=exhausted,
                 interleaved=interleaved)

if __name__ == "__main__":
    SCENARIOS[sys.argv[1]]()
    torch.cuda.synchronize()
    print("ROPE-SOURCE-OK", sys.argv[1], flush=True)
