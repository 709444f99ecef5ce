"""The attention planners' whole decision table (qserve_amd/csrc/attn_plan.h), pinned without a GPU.

tests/host/attn_plan_table.cpp prints one row per grid point of plan_attention (D), plan_append (A), plan_splits (S), plan_shared (P)
and fit_splits (F); its head has the columns.  tests/golden/attn_plan_table.json holds the table as it was before the planners moved
into the header: a SHA-256 of every group of rows (D per variant and fused_quant, S per batch, P per forced pair) and the slices
FULL names in full.  The rows the library can answer (qs_attention_plan: D with fused_quant = 0, without kflags / exp_flags;
qs_append_attention_plan: A; qs_append_attention_split_plan: S; qs_append_shared_plan: P with no forced count) are also compared
with the built library, so the header is what the library runs; and the grid must reach every cut of the planners.  A deliberate
change of a planner re-records the golden file:

    python tests/test_attn_plan_table_cpu.py TABLE.txt        (TABLE.txt = the program's output)
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
SOURCE = os.path.join(HERE, "host", "attn_plan_table.cpp")
GOLDEN = os.path.join(HERE, "golden", "attn_plan_table.json")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "g++"
KEY_TOKENS = {"D": 3, "A": 1, "S": 2, "P": 3, "F": 1}       # the leading tokens of a row that name its group
FULL = ("D 0 0 1 ", "A ", "S 1 ", "P 0 0 64 1 4 ", "F ")    # rows with these prefixes are recorded in full
CAP = 32 << 20                                               # the split-KV workspace
BLOCK = 4 * 32 * 130 * 4                                     # the four waves' record blocks of one workgroup and split: 65 KiB
FILL, MIN_PAGES, MAX_SPLITS = 512, 8, 64


def groups(text):
    out = OrderedDict()
    for line in text.splitlines():
        out.setdefault(" ".join(line.split(" ", KEY_TOKENS[line[0]])[:KEY_TOKENS[line[0]]]), []).append(line)
    return out


def digest(rows):
    return hashlib.sha256(("\n".join(rows) + "\n").encode()).hexdigest()


def encode(text):
    lines = text.splitlines()
    return {"sha256": {k: digest(r) for k, r in groups(text).items()},
            "full": {p: [l[len(p):] for l in lines if l.startswith(p)] for p in FULL}}


def parse(line):
    """'K a b c : x y z' -> (K, [a, b, c], [x, y, z])"""
    left, right = line.split(" : ")
    left = left.split()
    return left[0], [int(x) for x in left[1:]], [int(x) for x in right.split()]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("attn_plan") / "attn_plan_table")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", SOURCE, "-o", exe], check=True)
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout


def test_table_matches_the_recorded_one(table):
    with open(GOLDEN) as f:
        golden = json.load(f)
    now = encode(table)
    assert list(now["sha256"]) == list(golden["sha256"])
    for prefix in FULL:
        want, got = golden["full"][prefix], now["full"][prefix]
        assert len(got) == len(want), prefix
        for w, g in zip(want, got):
            assert g == w, f"rows '{prefix}...': recorded '{w}', now '{g}'"
    for key, rows in groups(table).items():
        if digest(rows) != golden["sha256"][key]:
            print("\n".join(rows))
            pytest.fail(f"group '{key}': its rows differ from the recorded ones (printed above)")


def rec_waves(tq, tokens, G):
    return min(4, max(1, -(-min(tq, tokens) * G // 32)))


def check_against_library(text, lib):
    """Every row a plan entry can answer, asked of `lib`; returns how many were."""
    p3, p5, p8 = (C.c_int * 3)(), (C.c_int * 5)(), (C.c_int * 8)()
    a3, a5, a8 = (C.cast(p, C.c_void_p) for p in (p3, p5, p8))
    asked = 0
    try:
        for line in text.splitlines():
            kind, a, r = parse(line)
            if kind == "D" and a[1] == 0:
                variant, _, int4, H, Hkv, mb, batch, ts = a
                lib.qs_set_attention_variant(variant)
                rc = lib.qs_attention_plan(batch, H, Hkv, mb, ts, int4, a3)
                if r[0] == 0:
                    assert rc == -2 and lib.qs_last_error().decode() == f"single_query_attention: num_heads/num_kv_heads = {H // Hkv} not in 1..8", line
                else:
                    assert rc == 0 and list(p3) == r[:3], (line, rc, list(p3))
            elif kind == "A":
                n, H, Hkv = a
                assert lib.qs_append_attention_plan(1, n, H, Hkv, a3) == 0
                assert list(p3) == (r if n else [0, 0, 0]), (line, list(p3))
            elif kind == "S":
                batch, n, H, Hkv, mp = a
                assert lib.qs_append_attention_split_plan(batch, n, mp, H, Hkv, 1, a5) == 0
                if batch == 0 or n == 0:
                    assert list(p5) == [0] * 5, (line, list(p5))
                else:
                    assert p5[3] == r[0] and p5[4] == (batch * Hkv * p5[1] * r[0] * BLOCK // 1024 if r[0] > 1 else 0), (line, list(p5))
            elif kind == "P" and a[0] == 0 and a[1] == 0:
                _, _, batch, ngroups, n, mgt, H, Hkv, ms, mp = a
                tq, q_tiles, waves, S, gq_tiles, P, rws, rwp, nbytes, unshared = r
                assert lib.qs_append_shared_plan(batch, n, ngroups, mgt, mp, ms, H, Hkv, 1, a8) == 0
                if P == 0:
                    want = [tq, q_tiles, waves, unshared, gq_tiles, 0, 4, batch * Hkv * q_tiles * unshared * BLOCK // 1024 if unshared > 1 else 0]
                else:
                    want = [tq, q_tiles, waves, S, gq_tiles, P, rws | (rwp << 8), (nbytes + 1023) // 1024]
                assert list(p8) == want, (line, list(p8))
            else:
                continue
            asked += 1
    finally:
        lib.qs_set_attention_variant(0)
    return asked


def test_library_answers_the_same(table, built_lib):
    from qserve_amd._lib import lib
    kinds = [l[0] for l in table.splitlines()]
    assert check_against_library(table, lib) >= kinds.count("D") // 2 + kinds.count("A") + kinds.count("S") + 5000


def test_grid_reaches_every_cut(table):
    """Each cut of the planners decides at least one row (stated on the rows' inputs, not on the planners' code)."""
    rows = [parse(l) for l in table.splitlines()]
    D = [(a, r) for k, a, r in rows if k == "D" and a[0] == 0]
    assert {r[0] for k, a, r in rows if k == "D"} == {0, 1, 2, 3}                                       # every family
    assert any(r[0] in (1, 2) and r[1] == 8 for a, r in D), "no row takes 8 splits, the chooser's last candidate"
    # pages / n < 2 ends the chooser's loop before n = 8 (4 .. 15 pages, fewer than 512 workgroups)
    assert any(r[0] in (1, 2) and 4 <= -(-a[7] // 64) < 16 and a[4] * a[6] < 512 for a, r in D)
    seen = set()
    for k, a, r in rows:
        if k != "S" or a[0] == 0 or a[1] == 0:
            continue
        batch, n, H, Hkv, mp = a
        base = batch * Hkv * -(-n // (128 // (H // Hkv)))
        if base >= FILL or mp < 128:
            assert r[0] == 1
            continue
        cuts = {"fill": FILL // base, "min_pages": -(-mp // 64) // MIN_PAGES, "workspace": CAP // (base * BLOCK), "max_splits": MAX_SPLITS}
        low = min(cuts.values())
        assert r[0] == max(low, 1), (a, r)
        binding = [c for c, v in cuts.items() if v == low]
        if len(binding) == 1:
            seen.add(binding[0])
    # (FILL / base alone never decides: 32 MiB hold 504 workgroups' blocks, so the workspace cut is never above it)
    assert seen == {"min_pages", "workspace", "max_splits"}, seen
    why = set()
    for k, a, r in rows:
        if k != "P":
            continue
        fp, fs, batch, ngroups, n, mgt, H, Hkv, ms, mp = a
        tq, q_tiles, waves, S, gq_tiles, P, rws, rwp, nbytes, unshared = r
        G = H // Hkv
        per_p = ngroups * gq_tiles * Hkv * rec_waves(tq, mgt, G) * BLOCK // 4
        per_s = batch * q_tiles * Hkv * rec_waves(tq, n, G) * BLOCK // 4
        if fp == -1 or (fp == 0 and (ngroups == batch or mp < 64)):
            assert P == 0
            why.add("P = 0: not asked to share")
        elif per_s > CAP:
            assert P == 0
            why.add("P = 0: one set of suffix records exceeds the workspace")
        elif fp > 0 and P == 0:
            assert CAP - per_s < per_p
            why.add("P = 0: the suffix set leaves no room for a set of prefix records")
        elif fp > 0 and fs > 0:
            assert nbytes == P * per_p + S * per_s <= CAP
            if P < min(fp, MAX_SPLITS) and S == min(fs, MAX_SPLITS):
                why.add("P yields")
            if P < min(fp, MAX_SPLITS) and S < min(fs, MAX_SPLITS):
                assert P == (CAP - per_s) // per_p and S == (CAP - P * per_p) // per_s, (a, r)
                why.add("P yields, then S yields")
    assert len(why) == 5, why


if __name__ == "__main__":
    with open(sys.argv[1]) as f, open(GOLDEN, "w") as g:
        json.dump(encode(f.read()), g, separators=(",", ":"))
        g.write("\n")
