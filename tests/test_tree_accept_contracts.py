"""Code-generation contracts of the device-side tail of tree verification, checked on the gfx950 assembly hipcc produces (CPU-only,
like tests/test_append_tree_contracts.py): tree_accept.hip assembles, holds exactly the accept kernel and the two instantiations of
the all-layers path commit (KV4, KV8), and none of them uses scratch memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qserve_amd", "csrc", "tree_accept.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("tree_accept_asm")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only"]
    r = subprocess.run([HIPCC, *flags, "-c", "-o", str(d / "accept.o"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([HIPCC, *flags, "-S", "-o", str(d / "accept.s"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(d / "accept.s").read()


def _kernels(text):
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)\n\s*s_endpgm", text, re.S | re.M)}


def _meta(text, name, key):
    return int(re.search(re.escape(name) + r".*?;\s*" + key + r":\s*(\d+)", text, re.S).group(1))


def test_the_file_holds_the_accept_kernel_and_the_two_movers(asm):
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(names) == 3
    assert len([n for n in names if "tree_accept_greedy_kernel" in n]) == 1
    movers = [n for n in names if "kv_commit_path_layers_kernel" in n]
    assert len(movers) == 2 and {bool(re.search(r"kernelILi64E", n)) for n in movers} == {True, False}      # 64 / 128 bytes per token


def test_no_kernel_uses_scratch(asm):
    ks = _kernels(asm)
    assert len(ks) == 3
    for name, body in ks.items():
        assert _meta(asm, name, "ScratchSize") == 0 and "scratch_" not in body, f"{name}: scratch"
