"""Code-generation contracts of the LoRA row kernels, checked on the gfx950 assembly hipcc produces (CPU-only, like
tests/test_constrain_rows_contracts.py): every LoRA .hip file - lora_rows.hip (the rows and the grouped form) and lora_prompt.hip -
assembles under the flags qserve_amd/build.py gives it, holds exactly the kernels its header comment documents, uses no scratch
memory, and keeps its LDS per workgroup under the bound the file states.  Nothing else of the assembly is looked at.  A file whose
kernels take dynamic LDS only (lora_prompt.hip) states a bound the assembly cannot show: that bound is checked against the constants
the launcher multiplies (PROMPT_TILE rows x LR_MAX_SEG x LR_MAX_RANK floats), not against the assembly."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from qserve_amd.build import SOURCE_FLAGS, SOURCES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qserve_amd", "csrc")
FILES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "lora_*.hip")))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
COUNTS = {"ONE": 1, "TWO": 2, "THREE": 3, "FOUR": 4, "FIVE": 5, "SIX": 6}
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_the_build_compiles_every_lora_file():
    assert FILES and all(f in SOURCES for f in FILES)


def _head(name):
    src = open(os.path.join(CSRC, name)).read()
    return src[:src.index("#include")]


def _documented(name):
    """The kernel name stems the header comment of `name` documents: the lines `//   <stem>_kernel ...`."""
    return re.findall(r"^//   (\w+_kernel)\b", _head(name), re.M)


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("lora_asm")
    out = {}
    for name in FILES:
        flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", *SOURCE_FLAGS.get(name, [])]
        for mode, ext in (("-c", ".o"), ("-S", ".s")):
            r = subprocess.run([HIPCC, *flags, mode, "-o", str(d / (name + ext)), os.path.join(CSRC, name)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
        out[name] = open(d / (name + ".s")).read()
    return out


def _meta(text, name, key):
    return int(re.search(re.escape(name) + r".*?;\s*" + key + r":\s*(\d+)", text, re.S).group(1))


@needs_hipcc
@pytest.mark.parametrize("name", FILES)
def test_the_file_holds_the_kernels_it_documents(asm, name):
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm[name], re.M)
    stems = _documented(name)
    count = COUNTS[re.search(r"holds (\w+) kernels", _head(name)).group(1)]
    assert len(stems) == count == len(set(stems)), (stems, count)
    # (a mangled name carries the stem behind its length: lora_shrink_kernel does not match lora_grouped_shrink_kernel)
    held = [[s for s in stems if f"{len(s)}{s}" in n] for n in names]
    assert all(len(h) == 1 for h in held), names
    assert {h[0] for h in held} == set(stems), names
    for s in stems:                                      # (one kernel per name, but for a name the header documents as a template: `name<...>`)
        assert re.search(re.escape(s) + "<", _head(name)) or sum(h == [s] for h in held) == 1, (s, names)


@needs_hipcc
@pytest.mark.parametrize("name", FILES)
def test_no_scratch_and_lds_under_the_stated_bound(asm, name):
    bound = int(re.search(r"The LDS bound of the file: ([\d ]+) bytes per workgroup", _head(name)).group(1).replace(" ", ""))
    assert 0 < bound <= 65536
    text, used = asm[name], {}
    for kernel in re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M):
        assert _meta(text, kernel, "ScratchSize") == 0, f"{kernel}: scratch"
        used[kernel] = _meta(text, kernel, "LDSByteSize")
    if any(used.values()):                               # static LDS: every kernel takes some, the largest exactly the bound
        for kernel, lds in used.items():
            assert 0 < lds <= bound, f"{kernel}: {lds} bytes of LDS, the file states {bound}"
        assert max(used.values()) == bound, f"{used}: the stated bound {bound} is not what the largest kernel takes"
    else:                                                # dynamic LDS only: what the launcher asks for at the largest R the rules admit
        src = open(os.path.join(CSRC, name)).read()
        assert "const size_t lds = (size_t)LP_TILE * R * sizeof(float);" in src and "LP_TILE = lora_plan::PROMPT_TILE;" in src
        consts = open(os.path.join(CSRC, "lora_common.h")).read() + open(os.path.join(CSRC, "lora_plan.h")).read()
        tile, seg, rank = (int(re.search(r"constexpr int " + k + r" = (\d+);", consts).group(1)) for k in ("PROMPT_TILE", "LR_MAX_SEG", "LR_MAX_RANK"))
        assert bound == tile * seg * rank * 4, f"the stated bound {bound} is not {tile} rows x {seg} x {rank} floats"
