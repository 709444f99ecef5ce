"""Code-generation contracts of the shared-prefix append attention kernels, checked on the gfx950 assembly hipcc produces (CPU-only,
like tests/test_append_split_contracts.py): the file assembles, both instantiations of the two-role kernel use no scratch memory,
keep two workgroups per CU and hold the 64 fp16 MFMAs of ONE key loop unrolled over the two LDS buffers (the split kernel's figures:
the role select did not instantiate the walk a second time), and the merge kernel does not spill."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qserve_amd", "csrc", "append_shared.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("append_shared_asm")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only"]
    # -c as well as -S: inline assembly is only checked by the assembler
    r = subprocess.run([HIPCC, *flags, "-c", "-o", str(d / "shared.o"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([HIPCC, *flags, "-S", "-o", str(d / "shared.s"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(d / "shared.s").read()


def _kernels(text):
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)\n\s*s_endpgm", text, re.S | re.M)}


def _meta(text, name, key):
    return int(re.search(re.escape(name) + r".*?;\s*" + key + r":\s*(\d+)", text, re.S).group(1))


def test_shared_kernels_keep_the_split_kernels_figures(asm):
    ks = {n: b for n, b in _kernels(asm).items() if "append_shared_kernel" in n}
    assert len(ks) == 2 and {bool(re.search(r"kernelILb1E", n)) for n in ks} == {True, False}        # KV4 and KV8
    for name, body in ks.items():
        assert _meta(asm, name, "ScratchSize") == 0 and "scratch_" not in body, f"{name}: scratch"
        assert _meta(asm, name, "Occupancy") == 2, name
        # two copies of the tile body (one per LDS buffer), 16 MFMAs for S^T = K Q^T and 16 for O^T = V^T P^T each
        n = len(re.findall(r"v_mfma_f32_32x32x16_f16", body))
        assert n == 64, f"{name}: {n} fp16 MFMAs"


def test_merge_kernel_does_not_spill(asm):
    ks = {n: b for n, b in _kernels(asm).items() if "append_shared_merge_kernel" in n}
    assert len(ks) == 1
    for name, body in ks.items():
        assert _meta(asm, name, "ScratchSize") == 0 and "scratch_" not in body
