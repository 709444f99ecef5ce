"""Code-generation contracts of the n-gram drafter, checked on the gfx950 assembly hipcc produces (CPU-only, like
tests/test_tree_accept_contracts.py): ngram_draft.hip assembles, holds exactly the two kernels it documents - the drafter and the
history append -, neither uses scratch memory, and the drafter's static LDS holds the staged history and stays within the budget the
file documents (DRAFT_LDS_BUDGET, itself below the 160 KiB of a compute unit)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qserve_amd", "csrc", "ngram_draft.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("ngram_draft_asm")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only"]
    r = subprocess.run([HIPCC, *flags, "-c", "-o", str(d / "draft.o"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([HIPCC, *flags, "-S", "-o", str(d / "draft.s"), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(d / "draft.s").read()


def _meta(text, name, key):
    return int(re.search(re.escape(name) + r".*?;\s*" + key + r":\s*(\d+)", text, re.S).group(1))


def _constant(name):
    """A `constexpr int NAME = a * b;` (or `= a;`) of the source file."""
    m = re.search(r"constexpr int " + name + r" = (\d+)(?: \* (\d+))?;", open(SRC).read())
    return int(m.group(1)) * int(m.group(2) or 1)


def test_the_file_holds_the_drafter_and_the_append(asm):
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    assert len(names) == 2
    assert len([n for n in names if "ngram_draft_tree_kernel" in n]) == 1 and len([n for n in names if "history_append_kernel" in n]) == 1
    assert "holds TWO kernels" in open(SRC).read()


def test_no_scratch_and_lds_within_the_documented_budget(asm):
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, re.M)
    for name in names:
        assert _meta(asm, name, "ScratchSize") == 0, f"{name}: scratch"
    budget, tokens = _constant("DRAFT_LDS_BUDGET"), _constant("DRAFT_LDS_TOKENS")
    assert budget <= 160 * 1024
    draft = next(n for n in names if "ngram_draft_tree_kernel" in n)
    assert 4 * tokens < _meta(asm, draft, "LDSByteSize") <= budget, "the drafter's static LDS"
    assert _meta(asm, next(n for n in names if "history_append_kernel" in n), "LDSByteSize") == 0
