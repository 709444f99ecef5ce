"""Code-generation contracts of the constrained-decoding kernels, checked on the gfx950 assembly hipcc produces (CPU-only, like
tests/test_penalize_rows_contracts.py): constrain_rows.hip assembles, holds exactly the three kernels its header comment documents,
uses no scratch memory and keeps its static LDS - one bit per class for the mask kernel, none for the other two - within a compute
unit's 160 KiB.  And the error paths of the wrappers of qserve_amd.constraints that need no device."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qserve_amd", "csrc", "constrain_rows.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("constrain_node_states_kernel", "constrain_rows_kernel", "constrain_advance_kernel")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("constrain_rows_asm")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only"]
    r = subprocess.run([HIPCC, *flags, "-c", "-o", str(d / "constrain.o"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([HIPCC, *flags, "-S", "-o", str(d / "constrain.s"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(d / "constrain.s").read()


def _meta(text, name, key):
    return int(re.search(re.escape(name) + r".*?;\s*" + key + r":\s*(\d+)", text, re.S).group(1))


@needs_hipcc
def test_the_file_holds_the_three_kernels_it_documents(asm):
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(names) == 3 and all(any(k in n for n in names) for k in KERNELS), names
    src = open(SRC).read()
    assert "holds THREE kernels" in src
    head = src[:src.index("#include")]
    assert all(re.search(r"^//\s+" + k + r"\b", head, re.M) for k in KERNELS)


@needs_hipcc
def test_no_scratch_and_lds_within_a_compute_unit(asm):
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M):
        assert _meta(asm, name, "ScratchSize") == 0, f"{name}: scratch"
        lds = _meta(asm, name, "LDSByteSize")
        assert lds <= 163840, f"{name}: LDS"
        assert (lds == 32768 // 8) == ("constrain_rows_kernel" in name), f"{name}: {lds} bytes of LDS (the mask: one bit per class)"


# ---- the wrappers' error paths that need no device ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mod(built_lib):
    from qserve_amd import constraints
    return constraints


def _tables(torch, V=16, S=2, C=3):
    return torch.zeros(V, dtype=torch.int16), torch.zeros((S, C), dtype=torch.int32)


def test_wrappers_refuse_wrong_types_and_shapes_before_any_device_call(mod):
    import torch
    tc, nx = _tables(torch)
    logits, rs = torch.zeros((2, 16), dtype=torch.float16), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(TypeError, match="token_class must be a torch.Tensor"):
        mod.constrain_rows(logits, rs, [0] * 16, nx)
    with pytest.raises(RuntimeError, match="expected scalar type torch.int16 for token_class"):
        mod.constrain_rows(logits, rs, tc.int(), nx)
    with pytest.raises(RuntimeError, match="expected scalar type torch.int32 for next"):
        mod.constrain_rows(logits, rs, tc, nx.long())
    with pytest.raises(RuntimeError, match=r"token_class must be \[n_vocab\] with n_vocab >= 8"):
        mod.constrain_rows(logits, rs, tc[:4], nx)
    with pytest.raises(RuntimeError, match=r"next must be \[S, C\]"):
        mod.constrain_rows(logits, rs, tc, torch.zeros((2, 40000), dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"next must be \[S, C\]"):
        mod.node_states(rs, torch.zeros((2, 3), dtype=torch.int64), torch.zeros(3, dtype=torch.int32), tc, nx.t())
    # (CPU tensors pass the shape checks and are refused by the device check, the last one before the library is called)
    with pytest.raises(RuntimeError, match="token_class must be on CUDA"):
        mod.constrain_rows(logits, rs, tc, nx)
    with pytest.raises(RuntimeError, match="token_class must be on CUDA"):
        mod.advance(rs, torch.zeros(2, dtype=torch.int64), tc, nx)


def test_token_dfa_checks_its_tensors(mod):
    import torch
    tc, nx = _tables(torch)
    d = mod.TokenDFA(tc, nx)
    assert (d.V, d.S, d.C) == (16, 2, 3) and mod.DEAD == -2
    with pytest.raises(ValueError, match="token_class must be int16"):
        mod.TokenDFA(tc.int(), nx)
    with pytest.raises(ValueError, match="next must be int32"):
        mod.TokenDFA(tc, nx.long())
    with pytest.raises(ValueError, match="next must be int32"):
        mod.TokenDFA(tc, torch.zeros((0, 3), dtype=torch.int32))


def test_library_refuses_bad_arguments_without_a_device(built_lib):
    """QS_EINVAL comes before any device call, so the C ABI itself can be asked here (addresses are never dereferenced)."""
    from qserve_amd._lib import lib
    ok = dict(logits=64, stride=16, V=16, rs=64, tc=64, nx=64, ns=3, S=2, C=3, rows=2)

    def rows(**kw):
        a = {**ok, **kw}
        return lib.qs_constrain_rows(a["logits"], a["stride"], a["V"], a["rs"], a["tc"], a["nx"], a["ns"], a["S"], a["C"], a["rows"], None)

    assert rows(rows=0) == 0
    for bad in (dict(logits=0), dict(rs=0), dict(tc=0), dict(nx=0), dict(V=7, stride=8), dict(V=(1 << 22) + 8, stride=(1 << 22) + 8),
                dict(stride=8), dict(stride=20), dict(C=0), dict(C=32769, ns=32769), dict(S=0), dict(ns=2), dict(rows=-1),
                dict(logits=72), dict(tc=72), dict(rs=66), dict(nx=66)):
        assert rows(**bad) == -1, bad
    assert b"constrain_rows" in lib.qs_last_error()

    def nodes(state=64, toks=64, par=64, n=4, batch=2, out=64, C=3, ns=3):
        return lib.qs_constrain_node_states(state, toks, par, 64, 16, 64, ns, 2, C, batch, n, out, None)

    assert nodes(batch=0) == 0
    for bad in (dict(state=0), dict(out=0), dict(toks=0), dict(par=0), dict(n=0), dict(n=65), dict(batch=-1), dict(toks=68), dict(state=66),
                dict(C=4)):
        assert nodes(**bad) == -1, bad

    def adv(state=64, ns=64, idx=64, lens=64, tok=64, n=4, m=4, batch=2):
        return lib.qs_constrain_advance(state, ns, idx, lens, tok, 64, 16, 64, 3, 2, 3, batch, n, m, None)

    assert adv(batch=0) == 0 and adv(batch=0, ns=0, idx=0, lens=0, n=1, m=1) == 0
    for bad in (dict(state=0), dict(tok=0), dict(idx=0), dict(m=0), dict(m=65), dict(n=0), dict(n=65), dict(batch=-1), dict(tok=68),
                dict(lens=66)):
        assert adv(**bad) == -1, bad
