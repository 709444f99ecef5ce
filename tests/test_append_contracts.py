"""Code-generation contracts of the append attention kernel, checked on the gfx950 assembly hipcc produces (CPU-only, like
tests/test_kernel_contracts.py): it assembles, uses no scratch memory (register spills), runs on the fp16 matrix cores, fits two
workgroups into one CU's LDS, and its key loop waits on the vector-memory queue only where the source says so."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qserve_amd", "csrc", "append_attention.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("append_asm")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only"]
    # -c as well as -S: inline assembly is only checked by the assembler
    r = subprocess.run([HIPCC, *flags, "-c", "-o", str(d / "append.o"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([HIPCC, *flags, "-S", "-o", str(d / "append.s"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(d / "append.s").read()


def _kernels(text):
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)\n\s*s_endpgm", text, re.S | re.M)}


def test_both_cache_types_are_instantiated_without_spills(asm):
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    scratch = [int(x) for x in re.findall(r"; ScratchSize: (\d+)", asm)]
    assert len(names) == len(scratch) == 2 and all("append_attention_kernel" in n for n in names)
    assert {bool(re.search(r"kernelILb1E", n)) for n in names} == {True, False}        # KV4 and KV8
    assert scratch == [0, 0], f"scratch bytes per lane: {dict(zip(names, scratch))}"
    assert "scratch_" not in "".join(_kernels(asm).values())


def test_products_run_on_the_fp16_matrix_cores(asm):
    for name, body in _kernels(asm).items():
        n = len(re.findall(r"v_mfma_f32_32x32x16_f16", body))
        # two copies of the tile body (one per LDS buffer), 16 MFMAs for S^T = K Q^T and 16 for O^T = V^T P^T each
        assert n == 64, f"{name}: {n} fp16 MFMAs"
        assert "ds_read_b64_tr_b16" in body and "global_load_lds_dwordx4" in body


def test_two_workgroups_fit_one_cu(asm):
    # the tile buffers are dynamic LDS: 2 x (K image + V image) of 64 keys x 128 dims fp16, requested by the launcher - through the
    # one launch tail of the append kernel pairs (append_walk.h launch_kernel_pair)
    assert re.search(r"return launch_kernel_pair<append_attention_kernel<true>, append_attention_kernel<false>>\(", open(SRC).read())
    tail = open(os.path.join(os.path.dirname(SRC), "append_walk.h")).read()
    assert re.search(r"constexpr int SMEM = 2 \* KS_BYTES \+ 2 \* VT_BYTES;", tail)
    assert re.search(r"hipLaunchKernelGGL\(KV4, grid, block, SMEM,", tail) and re.search(r"hipLaunchKernelGGL\(KV8, grid, block, SMEM,", tail)
    smem = 2 * (64 * 128 * 2) + 2 * (64 * 128 * 2)
    static = [int(x) for x in re.findall(r"; LDSByteSize: (\d+)", asm)]
    vgprs = [int(x) for x in re.findall(r"; NumVgprs: (\d+)", asm)]
    assert len(static) == 2 and len(vgprs) == 2
    for lds, vg in zip(static, vgprs):
        assert lds + smem <= LDS_PER_CU and 2 * (lds + smem) <= LDS_PER_CU
        assert 512 // ((vg + 7) // 8 * 8) >= 2, f"{vg} VGPRs: fewer than 2 waves per SIMD (two 4-wave workgroups per CU)"

