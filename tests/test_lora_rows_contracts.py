"""Code-generation contracts of the LoRA row kernels, checked on the gfx950 assembly hipcc produces (CPU-only, like
tests/test_constrain_rows_contracts.py): lora_rows.hip assembles, holds exactly the two kernels its header comment documents, uses no
scratch memory, and keeps its LDS per workgroup under the bound the file states.  Nothing else of the assembly is looked at."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qserve_amd", "csrc", "lora_rows.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("lora_shrink_kernel", "lora_expand_kernel")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("lora_rows_asm")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only"]
    r = subprocess.run([HIPCC, *flags, "-c", "-o", str(d / "lora.o"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([HIPCC, *flags, "-S", "-o", str(d / "lora.s"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(d / "lora.s").read()


def _meta(text, name, key):
    return int(re.search(re.escape(name) + r".*?;\s*" + key + r":\s*(\d+)", text, re.S).group(1))


@needs_hipcc
def test_the_file_holds_the_two_kernels_it_documents(asm):
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(names) == 2 and all(any(k in n for n in names) for k in KERNELS), names
    src = open(SRC).read()
    assert "holds TWO kernels" in src
    head = src[:src.index("#include")]
    assert all(re.search(r"^//\s+" + k + r"\b", head, re.M) for k in KERNELS)


@needs_hipcc
def test_no_scratch_and_lds_under_the_stated_bound(asm):
    head = open(SRC).read()
    head = head[:head.index("#include")]
    bound = int(re.search(r"The LDS bound of the file: ([\d ]+) bytes per workgroup", head).group(1).replace(" ", ""))
    assert 0 < bound <= 65536
    used = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M):
        assert _meta(asm, name, "ScratchSize") == 0, f"{name}: scratch"
        used[name] = _meta(asm, name, "LDSByteSize")
        assert 0 < used[name] <= bound, f"{name}: {used[name]} bytes of LDS, the file states {bound}"
    assert max(used.values()) == bound, f"{used}: the stated bound {bound} is not what the largest kernel takes"
