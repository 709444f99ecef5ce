"""Code-generation contracts of the tree-draft verification kernels, checked on the gfx950 assembly hipcc produces (CPU-only, like
tests/test_append_contracts.py and tests/test_append_split_contracts.py): the file assembles, every tree attention instantiation -
un-split and split-KV, KV4 and KV8 - keeps the linear kernels' figures (no scratch memory, two workgroups per CU, the 64 fp16 MFMAs
of the key loop unrolled over the two LDS buffers), and the path-commit kernel does not spill."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qserve_amd", "csrc", "append_tree.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("append_tree_asm")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only"]
    # -c as well as -S: inline assembly is only checked by the assembler
    r = subprocess.run([HIPCC, *flags, "-c", "-o", str(d / "tree.o"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([HIPCC, *flags, "-S", "-o", str(d / "tree.s"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(d / "tree.s").read()


def _kernels(text):
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)\n\s*s_endpgm", text, re.S | re.M)}


def _meta(text, name, key):
    return int(re.search(re.escape(name) + r".*?;\s*" + key + r":\s*(\d+)", text, re.S).group(1))


def test_the_file_holds_the_four_attention_kernels_and_the_two_movers(asm):
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(names) == 6
    for stem in ("append_tree_attention_kernel", "append_tree_attention_split_kernel"):
        mine = [n for n in names if stem + "I" in n]
        assert len(mine) == 2 and {bool(re.search(r"kernelILb1E", n)) for n in mine} == {True, False}, stem      # KV4 and KV8
    assert len([n for n in names if "kv_commit_path_kernel" in n]) == 2                                           # 64 / 128 bytes per token


def test_tree_attention_kernels_keep_the_linear_kernels_figures(asm):
    ks = {n: b for n, b in _kernels(asm).items() if "append_tree_attention" in n}
    assert len(ks) == 4
    for name, body in ks.items():
        assert _meta(asm, name, "ScratchSize") == 0 and "scratch_" not in body, f"{name}: scratch"
        assert _meta(asm, name, "Occupancy") == 2, name
        # two copies of the tile body (one per LDS buffer), 16 MFMAs for S^T = K Q^T and 16 for O^T = V^T P^T each
        n = len(re.findall(r"v_mfma_f32_32x32x16_f16", body))
        assert n == 64, f"{name}: {n} fp16 MFMAs"


def test_commit_kernel_does_not_spill(asm):
    ks = {n: b for n, b in _kernels(asm).items() if "kv_commit_path_kernel" in n}
    assert len(ks) == 2
    for name, body in ks.items():
        assert _meta(asm, name, "ScratchSize") == 0 and "scratch_" not in body
