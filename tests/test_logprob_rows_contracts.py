"""Code-generation contracts of the log-probability kernel, checked on the gfx950 assembly hipcc produces (CPU-only, like
tests/test_penalize_rows_contracts.py): logprob_rows.hip assembles, holds exactly the one kernel its header comment documents, uses no
scratch memory and keeps its static LDS within a compute unit's 160 KiB."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qserve_amd", "csrc", "logprob_rows.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("logprob_rows_asm")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only"]
    r = subprocess.run([HIPCC, *flags, "-c", "-o", str(d / "logprob.o"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([HIPCC, *flags, "-S", "-o", str(d / "logprob.s"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(d / "logprob.s").read()


def _meta(text, name, key):
    return int(re.search(re.escape(name) + r".*?;\s*" + key + r":\s*(\d+)", text, re.S).group(1))


def test_the_file_holds_the_one_kernel_it_documents(asm):
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(names) == 1 and "logprob_rows_kernel" in names[0]
    assert "holds ONE kernel" in open(SRC).read()


def test_no_scratch_and_lds_within_a_compute_unit(asm):
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M):
        assert _meta(asm, name, "ScratchSize") == 0, f"{name}: scratch"
        assert 0 < _meta(asm, name, "LDSByteSize") <= 163840, f"{name}: LDS"
