"""The W4A8 GEMM planner's whole decision table (qserve_amd/csrc/gemm_plan.h), pinned without a GPU.

tests/host/gemm_plan_table.cpp prints one row per (variant, per_group, act, M, N, K): the plan, the un-split fallback of a
K-sliced ring plan, the K-slice planes plan.  tests/golden/gemm_plan_table.json holds the table as it was before the three ring
searches shared one cost model (the default variant's rows in full, a SHA-256 of every other variant's rows); the rows the
library can answer (act = 0: qs_w4a8_gemm_plan, qs_w4a8_gemm_planes_plan) are also compared with the built library, so the
header is what the library runs.  A deliberate change of the planner re-records the golden file:

    python tests/test_gemm_plan_table_cpu.py TABLE.txt        (TABLE.txt = the program's output)
"""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys
from collections import OrderedDict

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "host", "gemm_plan_table.cpp")
GOLDEN = os.path.join(HERE, "golden", "gemm_plan_table.json")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"
FAMILY = {"S": 1, "P": 2, "R": 3, "T": 4, "W": 5}


def by_variant(text):
    """variant -> its rows (without the variant column), in the program's order"""
    out = OrderedDict()
    for line in text.splitlines():
        v, rest = line.split(" ", 1)
        out.setdefault(v, []).append(rest)
    return out


def digest(rows):
    return hashlib.sha256(("\n".join(rows) + "\n").encode()).hexdigest()


def default_rows(rows):
    """"per_group act N K" -> ["M plan fallback planes", ...]: the default variant's rows in full, compactly"""
    out = OrderedDict()
    for r in rows:
        pg, act, M, N, K, plan, fallback, planes = r.split()
        out.setdefault(f"{pg} {act} {N} {K}", []).append(f"{M} {plan} {fallback} {planes}")
    return out


def encode(text):
    t = by_variant(text)
    return {"variants": list(t), "default": default_rows(t["-1"]), "sha256": {v: digest(r) for v, r in t.items() if v != "-1"}}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_table")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", SOURCE, "-o", exe], check=True)
    return by_variant(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)


def test_table_matches_the_recorded_one(table):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert list(table) == golden["variants"]
    now = default_rows(table["-1"])
    assert list(now) == list(golden["default"])
    for key, rows in now.items():
        assert rows == golden["default"][key], f"default variant, per_group act N K = {key}"
    for v, rows in table.items():
        if v != "-1" and digest(rows) != golden["sha256"][v]:
            print(f"variant {v}: per_group act M N K plan fallback planes\n" + "\n".join(rows))
            pytest.fail(f"variant {v}: its rows differ from the recorded ones (printed above)")


def test_variants_are_not_inert(table):
    """The grid reaches what each named code switches: no named variant's rows equal the default's."""
    for v in ("2000", "2001", "3000", "3001", "3002", "3003", "4000", "4001", "4002", "4003", "4004"):
        assert table[v] != table["-1"], v


def test_library_answers_the_same(table):
    from qserve_amd._lib import lib
    p5, p4 = (C.c_int * 5)(), (C.c_int * 4)()
    a5, a4 = C.cast(p5, C.c_void_p), C.cast(p4, C.c_void_p)
    try:
        for v, rows in table.items():
            lib.qs_set_gemm_variant(int(v))
            for r in rows:
                pg, act, M, N, K, plan, _, planes = r.split()
                if act != "0":
                    continue
                pg, M, N, K = int(pg), int(M), int(N), int(K)
                rc = lib.qs_w4a8_gemm_plan(pg, M, N, K, a5)
                if plan == "X":
                    code = int(v) - 4100                        # QS_GEMM_RING_GEOMETRY_BASE + 100 * (ks - 1) + 10 * mt + wn
                    want = (f"w4a8 gemm: forced ring geometry mt={code % 100 // 10} wn={code % 10} ksplit={code // 100 + 1} "
                            f"does not fit M={M} N={N} K={K}")
                    assert rc == -1 and lib.qs_last_error().decode() == want, (v, r, rc, lib.qs_last_error())
                else:
                    want = [FAMILY[plan[0]]] + [int(x) for x in plan[1:].split(",") if x]
                    assert rc == 0 and list(p5) == want + [0] * (5 - len(want)), (v, r, rc, list(p5))
                assert lib.qs_w4a8_gemm_planes_plan(pg, M, N, K, a4) == 0
                want = [int(x) for x in planes.split(",")] if planes != "0" else [0] * 4
                assert list(p4) == want, (v, r, list(p4))
    finally:
        lib.qs_set_gemm_variant(-1)


if __name__ == "__main__":
    with open(sys.argv[1]) as f, open(GOLDEN, "w") as g:
        json.dump(encode(f.read()), g, separators=(",", ":"))
        g.write("\n")
