"""Contracts of the beam entries that need no GPU: the header declares both with their argument names in order, their argument
validation (before any HIP call), the lowering of beams.select / beams.move_rows onto them - through host-memory stand-ins written here
over the restatements of tests/_beam_cases.py -, and the code generation of beam_select.hip: it assembles for gfx950, holds the three
kernels its header comment documents and none of them uses scratch (private-segment) memory."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _beam_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qserve_amd", "csrc", "beam_select.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SELECT_ARGS = ["logits", "row_stride", "n_vocab", "cum", "finished", "tokens", "batch", "width", "parent", "next_token", "cum_out", "moved",
               "src_rows", "cand_ids", "cand_lp", "stream"]
MOVE_ARGS = ["parent", "batch", "bases", "row_bytes", "num", "error", "stream"]


@pytest.mark.parametrize("entry,args", [("qs_beam_select", SELECT_ARGS), ("qs_rows_move", MOVE_ARGS)])
def test_the_header_declares_the_entry_with_its_arguments_in_order(entry, args):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qserve_amd.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + entry + r"\s*\(([^;]*)\)\s*;", txt)
    assert m and [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == args
    from qserve_amd import _lib
    assert len(_lib.SIGNATURES[entry][1]) == len(args)
    assert "beam_select.hip" in __import__("qserve_amd.build", fromlist=["SOURCES"]).SOURCES


def test_select_argument_validation_without_gpu(built_lib):
    from qserve_amd._lib import lib
    ptrs = dict(logits=4096, cum=8192, finished=12288, tokens=16384, parent=20480, next_token=24576, cum_out=28672, moved=32768,
                src_rows=36864, cand_ids=40960, cand_lp=45056)

    def select(stride=1000, n=1000, batch=8, width=4, **change):
        p = {**ptrs, **change}
        return lib.qs_beam_select(p["logits"], stride, n, p["cum"], p["finished"], p["tokens"], batch, width, p["parent"], p["next_token"],
                                  p["cum_out"], p["moved"], p["src_rows"], p["cand_ids"], p["cand_lp"], None)

    for name in ptrs:
        if name not in ("moved", "src_rows"):
            assert select(**{name: None}) == -1 and b"null pointer" in lib.qs_last_error(), name
    for width in (0, -1, 33):
        assert select(width=width, batch=0) == -1 and b"width=" in lib.qs_last_error()
    assert select(batch=9) == -1 and b"not a multiple of width" in lib.qs_last_error()
    assert select(batch=-4) == -1 and select(batch=65536, width=32) == -1 and b"batch=65536" in lib.qs_last_error()
    assert select(n=7, stride=8) == -1 and select(n=(1 << 22) + 8, stride=(1 << 22) + 8) == -1 and b"n_vocab=" in lib.qs_last_error()
    assert select(stride=992) == -1 and select(n=1001, stride=1004) == -1 and b"multiple of 8" in lib.qs_last_error()
    assert select(cum_out=ptrs["cum"]) == -1 and b"must not alias cum" in lib.qs_last_error()
    assert select(logits=4104) == -1 and b"16-byte" in lib.qs_last_error()
    for name in ("tokens", "next_token"):
        assert select(**{name: ptrs[name] + 4}) == -1 and b"8-byte" in lib.qs_last_error(), name
    for name in ("cum", "finished", "parent", "cum_out", "moved", "src_rows", "cand_ids", "cand_lp"):
        assert select(**{name: ptrs[name] + 2}) == -1 and b"4-byte" in lib.qs_last_error(), name
    assert select(batch=0) == 0 and select(batch=0, moved=None, src_rows=None) == 0          # nothing to do: no launch


def test_move_argument_validation_without_gpu(built_lib):
    import ctypes
    from qserve_amd._lib import lib

    def move(parent=4096, batch=0, bases=(8192, 12288), sizes=(4, 20), num=None, error=16384):
        b = (ctypes.c_void_p * 16)(*bases) if bases is not None else None
        s = (ctypes.c_int64 * 16)(*sizes) if sizes is not None else None
        return lib.qs_rows_move(parent, batch, b, s, len(bases or ()) if num is None else num, error, None)

    assert move() == 0 and move(bases=(), sizes=()) == 0                    # batch == 0: no launch
    assert move(batch=4, bases=(), sizes=()) == 0                           # no tensors: no launch
    assert move(parent=None) == -1 and b"null pointer" in lib.qs_last_error()
    assert move(error=None) == -1 and b"null pointer" in lib.qs_last_error()
    assert move(parent=4098) == -1 and b"4-byte" in lib.qs_last_error()
    assert move(batch=-1) == -1 and move(batch=65536) == -1 and b"batch=65536" in lib.qs_last_error()
    assert move(num=17) == -1 and move(num=-1) == -1 and b"num=-1" in lib.qs_last_error()
    assert move(bases=None, num=1) == -1 and move(sizes=None, num=1) == -1 and b"null pointer" in lib.qs_last_error()
    assert move(bases=(8192, 0)) == -1 and b"tensor 1" in lib.qs_last_error()
    assert move(sizes=(0, 20)) == -1 and b"tensor 0" in lib.qs_last_error()
    assert move(sizes=(4, (1 << 31) + 1)) == -1 and b"tensor 1" in lib.qs_last_error()


# ---- the entries over host memory -----------------------------------------------------------------------------------------------------
def _fake_select(logits, row_stride, n, cum, finished, tokens, batch, width, parent, next_token, cum_out, moved, src_rows, cand_ids, cand_lp,
                 stream):
    import _fake_abi as F
    F.CALLS.append(("qs_beam_select", batch, width, n, row_stride, bool(moved), bool(src_rows)))
    x = F._strided_rows(logits, batch, row_stride, n, np.float16)
    c, fin, tok = F._arr(cum, (batch,), np.float32), F._arr(finished, (batch,), np.int32), F._arr(tokens, (batch,), np.int64)
    ids, lp = K.candidates_oracle(x, c, fin, width)
    F._arr(cand_ids, (batch, width), np.int32)[:] = ids
    F._arr(cand_lp, (batch, width), np.float32)[:] = lp
    res = K.merge_loop(c, fin, tok, ids, lp.astype(np.float32), width)
    for addr, key, dt in ((parent, "parent", np.int32), (next_token, "next_token", np.int64), (cum_out, "cum_out", np.float32),
                          (moved, "moved", np.int32), (src_rows, "src_rows", np.int32)):
        if addr:
            F._arr(addr, (batch,), dt)[:] = res[key]
    return 0


def _fake_move(parent, batch, bases, row_bytes, num, error, stream):
    import _fake_abi as F
    F.CALLS.append(("qs_rows_move", batch, num, [int(row_bytes[i]) for i in range(num)]))
    views = [F._arr(bases[i], (batch, int(row_bytes[i])), np.uint8) for i in range(num)]
    out, err = K.move_loop(F._arr(parent, (batch,), np.int32), views)
    for v, o in zip(views, out):
        v[:] = o
    if err:
        F._arr(error, (1,), np.int32)[0] = 1
    return 0


def install(monkeypatch):
    """tests/_fake_abi.py's stand-ins, the two above, and host tensors accepted by qserve_amd.beams -> the call list."""
    import _fake_abi as F
    import qserve_amd.beams as beamsmod
    from qserve_amd._lib import lib
    calls = F.install(monkeypatch)
    monkeypatch.setattr(lib, "qs_beam_select", _fake_select, raising=True)
    monkeypatch.setattr(lib, "qs_rows_move", _fake_move, raising=True)
    import qserve_amd.backend._util as U
    for attr in ("stream", "expect", "guard"):
        monkeypatch.setattr(beamsmod, attr, getattr(U, attr))               # (already the host forms: F.install patched _util)
    return calls


def test_select_lowers_onto_the_entry(built_lib, monkeypatch):
    from qserve_amd import beams
    calls = install(monkeypatch)
    case = K.named_cases()["frozen_rows"]
    buf = torch.zeros((6, 16), dtype=torch.float16)
    buf[:, :9] = torch.from_numpy(case["logits"])
    args = [torch.from_numpy(case[k].copy()) for k in ("cum", "finished", "tokens")]
    res = beams.select(buf[:, :9], *args, 3)
    assert calls[-1] == ("qs_beam_select", 6, 3, 9, 16, True, True)
    ids, lp = K.candidates_oracle(case["logits"], case["cum"], case["finished"], 3)
    want = K.merge_loop(case["cum"], case["finished"], case["tokens"], ids, lp.astype(np.float32), 3)
    for key, t in zip(("parent", "next_token", "cum_out", "moved", "src_rows"), res):
        assert np.array_equal(t.numpy(), want[key]) and t.numpy().dtype == want[key].dtype, key
    assert np.array_equal(res[5].numpy(), ids)
    out = list(res)
    out[3] = out[4] = None                                                  # moved and src_rows are optional
    beams.select(buf[:, :9], *args, 3, out=tuple(out))
    assert calls[-1] == ("qs_beam_select", 6, 3, 9, 16, False, False)
    n = len(calls)
    f32, i32 = (lambda *s: torch.zeros(s, dtype=torch.float32)), (lambda *s: torch.zeros(s, dtype=torch.int32))   # noqa: E731
    cum, fin, tok = args
    for match, call in (("width=4", lambda: beams.select(buf[:, :9], cum, fin, tok, 4)), ("width=0", lambda: beams.select(buf[:, :9], cum, fin, tok, 0)),
                        ("width=33", lambda: beams.select(buf[:, :9], cum, fin, tok, 33)),
                        ("cum must be", lambda: beams.select(buf[:, :9], f32(5), fin, tok, 3)),
                        ("for cum", lambda: beams.select(buf[:, :9], cum.double(), fin, tok, 3)),
                        ("for finished", lambda: beams.select(buf[:, :9], cum, fin.long(), tok, 3)),
                        ("for tokens", lambda: beams.select(buf[:, :9], cum, fin, tok.int(), 3)),
                        ("row stride", lambda: beams.select(torch.zeros((6, 9), dtype=torch.float16), cum, fin, tok, 3)),
                        ("out is", lambda: beams.select(buf[:, :9], cum, fin, tok, 3, out=res[:6])),
                        ("out cand_ids must be", lambda: beams.select(buf[:, :9], cum, fin, tok, 3, out=(*res[:5], i32(6, 4), res[6]))),
                        ("must not be cum", lambda: beams.select(buf[:, :9], cum, fin, tok, 3, out=(res[0], res[1], cum, *res[3:])))):
        with pytest.raises(RuntimeError, match=match):
            call()
    assert len(calls) == n


def test_move_rows_lowers_onto_the_entry(built_lib, monkeypatch):
    from qserve_amd import beams
    calls = install(monkeypatch)
    g = torch.Generator().manual_seed(3)
    tensors = [torch.randint(0, 100, (4,), generator=g, dtype=torch.int32), torch.randint(0, 100, (4, 5), generator=g, dtype=torch.int32),
               torch.randint(0, 100, (4, 2, 3), generator=g, dtype=torch.int64)]
    before = [t.numpy().copy() for t in tensors]
    err = torch.zeros((1,), dtype=torch.int32)
    beams.move_rows(torch.tensor([0, 0, 3, 3], dtype=torch.int32), tensors, err)
    assert calls[-1] == ("qs_rows_move", 4, 3, [4, 20, 48])
    want, _ = K.move_loop([0, 0, 3, 3], before)
    assert int(err) == 0 and all(np.array_equal(t.numpy(), w) for t, w in zip(tensors, want))
    beams.move_rows(torch.tensor([1, 2, 2, 3], dtype=torch.int32), tensors, err)
    assert int(err) == 1
    n = len(calls)
    par = torch.zeros((4,), dtype=torch.int32)
    for match, call in (("for parent", lambda: beams.move_rows(par.long(), tensors, err)), ("parent must be", lambda: beams.move_rows(par.view(2, 2), tensors, err)),
                        ("error must be", lambda: beams.move_rows(par, tensors, torch.zeros((2,), dtype=torch.int32))),
                        ("at most 16", lambda: beams.move_rows(par, tensors * 6, err)),
                        (r"tensors\[0\] must be", lambda: beams.move_rows(par, [torch.zeros((5, 2))], err)),
                        (r"tensors\[0\] must be", lambda: beams.move_rows(par, [torch.zeros((4, 4))[:, :2]], err))):
        with pytest.raises(RuntimeError, match=match):
            call()
    assert len(calls) == n


def test_rank_orders_by_the_length_penalised_score():
    from qserve_amd import beams
    order, scores = beams.rank([-4.0, -3.0, -4.0, float("-inf")], [4, 2, 0, 3], 1.0)
    assert scores[:3] == [-1.0, -1.5, -4.0] and order == [0, 1, 2, 3]
    order, _ = beams.rank([-4.0, -3.0, -4.0], [4, 2, 4], 0.0)
    assert order == [1, 0, 2]                                               # the raw sums, ties by row
    order, scores = beams.rank([-6.0, -4.0], [9, 4], 0.5)
    assert scores == [-2.0, -2.0] and order == [0, 1]


# ---- code generation ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("beam_select_asm")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only"]
    r = subprocess.run([HIPCC, *flags, "-S", "-o", str(d / "beam.s"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(d / "beam.s").read()


def _meta(text, name, key):
    return int(re.search(re.escape(name) + r".*?;\s*" + key + r":\s*(\d+)", text, re.S).group(1))


def test_the_file_holds_the_three_kernels_it_documents_without_spills(asm):
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(names) == 3 and all(any(k in n for n in names) for k in ("beam_candidates_kernel", "beam_merge_kernel", "rows_move_kernel"))
    assert "holds THREE kernels" in open(SRC).read()
    for name in names:
        assert _meta(asm, name, "ScratchSize") == 0, f"{name}: private-segment (spill) bytes"
        assert _meta(asm, name, "LDSByteSize") <= 163840, f"{name}: LDS"
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", asm.split(".amdhsa_kernel " + name)[1]).group(1)) == 0
