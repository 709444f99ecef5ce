"""Contracts of the stop rule that need no GPU: the header declares the entry, `qs_stop_update`'s argument validation (which happens
before any HIP call), the argument checks of qserve_amd.stopping and its lowering onto the C ABI (through the host-memory stand-in of
tests/_fake_abi.py, with the entry monkeypatched in), and the code-generation contracts of stop_update.hip on the gfx950 assembly hipcc
produces: it holds the one kernel its header comment documents, uses no scratch memory and no LDS."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from _stop_cases import named_cases, restate_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qserve_amd", "csrc", "stop_update.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_the_header_declares_the_entry():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qserve_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+qs_stop_update\s*\(", txt)
    from qserve_amd import _lib
    assert len(_lib.SIGNATURES["qs_stop_update"][1]) == 22


def test_argument_validation_without_gpu(built_lib):
    from qserve_amd._lib import lib

    def call(history=4096, hstride=64, cap=64, lengths=8192, prompt=None, nodes=16384, idx=20480, lens=24576, out_lens=None, nxt=28672,
             last=None, seqs=32768, slens=36864, limits=None, fin=40960, batch=2, n=4, max_accept=4, S=2, W=3, root=0):
        return lib.qs_stop_update(history, hstride, cap, lengths, prompt, nodes, idx, lens, out_lens, nxt, last, seqs, slens, limits, fin,
                                  batch, n, max_accept, S, W, root, None)

    for bad in ("history", "lengths", "nxt", "fin"):
        assert call(**{bad: None}) == -1 and b"null pointer" in lib.qs_last_error(), bad
    assert call(lens=None) == -1 and b"out_lens" in lib.qs_last_error()
    assert call(lens=None, out_lens=24576, batch=0) == 0
    assert call(seqs=None) == -1 and call(slens=None) == -1 and b"num_stops=2" in lib.qs_last_error()
    assert call(seqs=None, slens=None, S=0, batch=0) == 0
    assert call(S=-1) == -1 and call(S=33) == -1 and b"num_stops=33" in lib.qs_last_error()
    assert call(W=0) == -1 and call(W=9) == -1 and b"stop_width=9" in lib.qs_last_error()
    assert call(n=0) == -1 and call(n=65) == -1 and b"n=65" in lib.qs_last_error()
    assert call(max_accept=0) == -1 and call(max_accept=65) == -1 and b"max_accept=65" in lib.qs_last_error()
    assert call(nodes=None) == -1 and b"node_tokens is null with n=4" in lib.qs_last_error()
    assert call(nodes=None, n=1, batch=0) == 0
    assert call(idx=None) == -1 and b"accept_idx is null" in lib.qs_last_error()
    assert call(idx=None, max_accept=1, batch=0) == 0
    assert call(cap=0) == -1 and b"cap=0" in lib.qs_last_error()
    assert call(hstride=63) == -1 and b"hist_stride=63" in lib.qs_last_error()
    assert call(root=2) == -1 and b"check_root=2" in lib.qs_last_error()
    assert call(batch=-1) == -1
    for name in ("history", "lengths", "prompt", "idx", "lens", "seqs", "slens", "limits", "fin"):
        assert call(**{name: 8194}) == -1 and b"4-byte" in lib.qs_last_error(), name
    for name in ("nodes", "nxt", "last"):
        assert call(**{name: 16388}) == -1 and b"8-byte" in lib.qs_last_error(), name
    assert call(batch=0) == 0                                               # nothing to do: no launch
    assert call(batch=0, S=32, W=8, n=64, max_accept=64, root=1) == 0       # the largest table, tree and path


def _host_args(B=3, n=4):
    return dict(history=torch.zeros((B, 16), dtype=torch.int32), lengths=torch.zeros((B,), dtype=torch.int32),
                next_token=torch.zeros((B,), dtype=torch.int64), finished=torch.zeros((B,), dtype=torch.int32),
                stop_seqs=torch.zeros((2, 3), dtype=torch.int32), stop_lens=torch.zeros((2,), dtype=torch.int32),
                node_tokens=torch.zeros((B, n), dtype=torch.int64), accept_idx=torch.zeros((B, n), dtype=torch.int32),
                accept_lens=torch.zeros((B,), dtype=torch.int32))


def test_stopping_argument_checks(built_lib):
    """Wrong dtypes, shapes and combinations are reported with the argument's name before anything is launched (CPU tensors: the device
    check comes last)."""
    from qserve_amd import stopping as S
    ok = _host_args()

    def bad(match, **change):
        with pytest.raises(RuntimeError, match=match):
            S.stop_update(**{**ok, **change})

    bad("history", history=ok["history"].long())
    bad("history must be", history=ok["history"].t())
    bad("lengths must be", lengths=ok["lengths"][:2])
    bad("next_token", next_token=ok["next_token"].int())
    bad("finished must be", finished=torch.zeros((4,), dtype=torch.int32))
    bad("come together", stop_lens=None)
    bad("stop_seqs must be", stop_seqs=torch.zeros((33, 3), dtype=torch.int32), stop_lens=torch.zeros((33,), dtype=torch.int32))
    bad("stop_seqs must be", stop_seqs=torch.zeros((2, 9), dtype=torch.int32))
    bad("stop_lens must be", stop_lens=torch.zeros((3,), dtype=torch.int32))
    bad("limit_lens", limit_lens=torch.zeros((3,), dtype=torch.int64))
    bad("prompt_lens must be", prompt_lens=torch.zeros((2,), dtype=torch.int32))
    bad("last_row", last_row=torch.zeros((3,), dtype=torch.int32))
    bad("come together", accept_idx=None)
    bad("node_tokens", node_tokens=ok["node_tokens"].int())
    bad("node_tokens must be", node_tokens=torch.zeros((3, 65), dtype=torch.int64))
    bad("accept_idx must be", accept_idx=torch.zeros((2, 4), dtype=torch.int32))
    bad("needs its accept_lens", accept_lens=None)
    bad("history must be on CUDA")                                           # everything else is right: the device is what is left


def _fake_stop_update(history, hist_stride, cap, lengths, prompt_lens, node_tokens, accept_idx, accept_lens, out_lens, next_token, last_row,
                      stop_seqs, stop_lens, limit_lens, finished, batch, n, max_accept, S, W, check_root, stream):
    """qs_stop_update over host memory: re-materialise the arrays from the addresses and apply the loop restatement."""
    import _fake_abi as F
    F.CALLS.append(("qs_stop_update", batch, n, max_accept, S, W, check_root, hist_stride, cap))
    arr = lambda a, shape, dt: F._arr(a, shape, dt) if a else None   # noqa: E731
    views = dict(lengths=arr(lengths, (batch,), np.int32), prompt_lens=arr(prompt_lens, (batch,), np.int32),
                 node_tokens=arr(node_tokens, (batch, n), np.int64), accept_idx=arr(accept_idx, (batch, max_accept), np.int32),
                 accept_lens=arr(accept_lens, (batch,), np.int32), next_token=arr(next_token, (batch,), np.int64),
                 stop_seqs=arr(stop_seqs, (S, W), np.int32), stop_lens=arr(stop_lens, (S,), np.int32), limit_lens=arr(limit_lens, (batch,), np.int32),
                 finished=arr(finished, (batch,), np.int32))
    views["last_row"] = arr(last_row, (batch,), np.int64) if last_row else np.zeros((batch,), np.int64)
    out = restate_loop(dict(views, history=F._strided_rows(history, batch, hist_stride, cap, np.int32), cap=cap, n=n, max_accept=max_accept,
                            check_root=check_root))
    (views["accept_lens"] if accept_lens else F._arr(out_lens, (batch,), np.int32))[:] = out["accept_lens"]
    views["next_token"][:], views["finished"][:] = out["next_token"], out["finished"]
    if last_row:
        views["last_row"][:] = out["last_row"]
    return 0


def test_the_wrapper_lowers_onto_the_abi(built_lib, monkeypatch):
    """qserve_amd.stopping over the host-memory stand-in of the C ABI: the padded history's stride, null pointers for the optional
    arguments, in-place accept_lens against out_lens, n / max_accept / S / W from the shapes and check_root arrive as the header orders
    them."""
    import _fake_abi as F
    from qserve_amd import stopping as S
    from qserve_amd._lib import lib
    calls = F.install(monkeypatch)
    monkeypatch.setattr(lib, "qs_stop_update", _fake_stop_update, raising=False)
    import qserve_amd.backend._util as U
    for attr in ("stream", "expect", "guard"):
        monkeypatch.setattr(S, attr, getattr(U, attr))
    t = lambda a: None if a is None else torch.from_numpy(a.copy())   # noqa: E731
    # a verification over a padded history
    case = named_cases()["tree12_state"]
    want = restate_loop(case)
    arg = {k: t(case[k]) for k in ("lengths", "next_token", "finished", "stop_seqs", "stop_lens", "limit_lens", "prompt_lens", "node_tokens",
                                   "accept_idx", "accept_lens", "last_row")}
    store = t(case["history"])
    res = S.stop_update(store[:, :case["cap"]], **arg)
    assert calls[-1] == ("qs_stop_update", 8, 12, 12, 3, 3, 0, 56, 48) and res is arg["accept_lens"]
    for key in want:
        assert np.array_equal(arg[key].numpy(), want[key]), key
    # a plain step: no draft, k goes to a tensor the wrapper creates
    case = named_cases()["step"]
    want = restate_loop(case)
    arg = {k: t(case[k]) for k in ("lengths", "next_token", "finished", "stop_seqs", "stop_lens", "limit_lens", "prompt_lens")}
    res = S.stop_update(t(case["history"]), **arg)
    assert calls[-1] == ("qs_stop_update", 7, 1, 1, 3, 3, 0, 48, 48)
    assert res.dtype == torch.int32 and np.array_equal(res.numpy(), want["accept_lens"])
    assert np.array_equal(arg["next_token"].numpy(), want["next_token"]) and np.array_equal(arg["finished"].numpy(), want["finished"])
    # check_root, no table
    case = named_cases()["root"]
    arg = {k: t(case[k]) for k in ("lengths", "next_token", "finished", "limit_lens", "prompt_lens", "node_tokens", "accept_idx", "accept_lens")}
    S.stop_update(t(case["history"]), check_root=True, **arg)
    assert calls[-1][1:7] == (6, 12, 12, 0, 1, 1)
    # B == 0 returns at once
    n_calls = len(calls)
    S.stop_update(torch.zeros((0, 16), dtype=torch.int32), torch.zeros((0,), dtype=torch.int32), torch.zeros((0,), dtype=torch.int64),
                  torch.zeros((0,), dtype=torch.int32))
    assert len(calls) == n_calls


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("stop_update_asm")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only"]
    r = subprocess.run([HIPCC, *flags, "-S", "-o", str(d / "stop.s"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(d / "stop.s").read()


def _meta(text, name, key):
    return int(re.search(re.escape(name) + r".*?;\s*" + key + r":\s*(\d+)", text, re.S).group(1))


def test_one_kernel_without_scratch_or_lds(asm):
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(names) == 1 and "stop_update_kernel" in names[0]
    assert "holds ONE kernel" in open(SRC).read()
    assert _meta(asm, names[0], "ScratchSize") == 0 and _meta(asm, names[0], "LDSByteSize") == 0
