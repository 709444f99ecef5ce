"""The argument checks of the six page pool entries, pinned without a GPU: qs_pages_reserve, qs_pages_release, qs_pages_reserve_refs,
qs_pages_hold, qs_pages_unhold and qs_pages_fork.

Every call below breaks the contract in one place (thirty and more per entry: a null or misaligned pointer per argument, the optional
ones included, and every range check) or in two (the FIRST broken check must answer, so the order of the checks is pinned too) or asks
for nothing (a no-op: 0, no text), and returns before any device call - the pointers are small integers nobody may follow.
tests/golden/page_entry_errors.json holds each call's return code and the exact qs_last_error() text as the library gave them before
the entries shared one argument function.  The *_contracts.py tests assert substrings of some of these texts; this pins all of every
text.  A deliberate change of a message re-records it:

    python tests/test_page_entry_errors_cpu.py
"""
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "page_entry_errors.json")

# the pool state every entry takes first (int32 arrays at multiples of 4, the two int64 arrays at multiples of 8), then each entry's own
BASE = dict(fl=16, cnt=20, ids=24, own=28, stv=32, err=36, lt=40, lb=48, len=64, xr=68, fin=72, mask=76, refs=80, scr=84, take=88, src=92,
            xids=96, nx=2, srows=100, B=2, mb=4, L=2, N=8, pb=256, extra=1)
STATE = ("fl", "cnt", "ids", "own", "stv", "err", "lt", "lb")
COMMON_FAULTS = [dict(fl=0), dict(cnt=0), dict(ids=0), dict(own=0), dict(stv=0), dict(err=0), dict(lt=0), dict(lb=0),
                 dict(N=0), dict(N=-3), dict(mb=0), dict(L=0), dict(L=-1), dict(pb=0), dict(N=1 << 29), dict(B=-1), dict(B=1025),
                 dict(B=1024, mb=1 << 20),
                 dict(fl=18), dict(cnt=21), dict(ids=26), dict(own=29), dict(stv=34), dict(err=37), dict(lt=44), dict(lb=52),
                 # two faults: the earlier check answers
                 dict(lb=0, N=0), dict(N=0, mb=0), dict(mb=0, L=0), dict(L=0, pb=0), dict(pb=0, B=-1), dict(N=1 << 29, B=1025),
                 dict(B=1025, fl=18), dict(B=1024, mb=1 << 20, own=29), dict(stv=34, lt=44), dict(lb=52, lt=0)]
RESERVE_FAULTS = [dict(len=0), dict(len=66), dict(xr=70), dict(fin=73), dict(extra=-1),
                  dict(len=0, extra=-1), dict(xr=70, extra=-1), dict(lt=44, extra=-1), dict(extra=-1, B=0), dict(fin=73, lb=52)]
RESERVE_NOOPS = [dict(B=0), dict(B=0, xr=0, fin=0), dict(B=0, extra=0, mb=1 << 30)]
RELEASE_FAULTS = [dict(mask=0), dict(mask=78), dict(mask=0, N=0), dict(mask=78, lt=44), dict(mask=78, B=1025)]
RELEASE_NOOPS = [dict(B=0)]
REFS_FAULTS = [dict(refs=0), dict(refs=82), dict(refs=0, extra=-1), dict(refs=82, extra=-1), dict(xr=70, refs=0), dict(lb=52, refs=0),
               dict(refs=0, B=0)]
HOLD_FAULTS = [dict(take=0), dict(take=90), dict(src=0), dict(src=94), dict(refs=0), dict(refs=82), dict(scr=0), dict(scr=85), dict(xids=0),
               dict(xids=97), dict(nx=-1), dict(nx=9), dict(xids=97, nx=0),
               dict(take=0, src=0), dict(src=0, refs=0), dict(src=0, lt=44), dict(src=94, refs=0), dict(refs=0, scr=0), dict(scr=0, nx=-1),
               dict(nx=9, xids=0), dict(xids=0, refs=82), dict(nx=-1, B=0), dict(lb=52, src=0)]
HOLD_NOOPS = [dict(B=0, nx=0), dict(B=0, nx=0, xids=0)]
UNHOLD_FAULTS = [dict(mask=0), dict(mask=78), dict(refs=0), dict(refs=82), dict(scr=0), dict(scr=85), dict(xids=0), dict(xids=97), dict(nx=-1),
                 dict(nx=9), dict(xids=97, nx=0),
                 dict(mask=0, refs=0), dict(mask=78, refs=0), dict(refs=0, scr=0), dict(scr=0, nx=9), dict(nx=9, xids=0), dict(xids=0, scr=85),
                 dict(nx=-1, B=0), dict(lt=44, scr=0)]
UNHOLD_NOOPS = [dict(B=0, nx=0), dict(B=0, nx=0, xids=0)]
FORK_FAULTS = [dict(srows=0), dict(srows=102), dict(len=0), dict(len=66), dict(fin=73), dict(refs=0), dict(refs=82),
               dict(srows=0, len=0), dict(len=0, refs=0), dict(len=0, fin=73), dict(len=66, refs=0), dict(lb=52, len=0), dict(refs=0, B=0),
               dict(len=0, B=1025)]
FORK_NOOPS = [dict(B=0), dict(B=0, fin=0)]


def _call(lib, entry, a):
    state = tuple(a[k] for k in STATE)
    geom = (a["B"], a["mb"], a["L"], a["N"], a["pb"])
    if entry == "qs_pages_reserve":
        return lib.qs_pages_reserve(*state, a["len"], a["xr"], a["fin"], *geom, a["extra"], None)
    if entry == "qs_pages_release":
        return lib.qs_pages_release(*state, a["mask"], *geom, None)
    if entry == "qs_pages_reserve_refs":
        return lib.qs_pages_reserve_refs(*state, a["refs"], a["len"], a["xr"], a["fin"], *geom, a["extra"], None)
    if entry == "qs_pages_hold":
        return lib.qs_pages_hold(*state, a["refs"], a["scr"], a["take"], a["src"], a["xids"], a["nx"], *geom, None)
    if entry == "qs_pages_unhold":
        return lib.qs_pages_unhold(*state, a["refs"], a["scr"], a["mask"], a["xids"], a["nx"], *geom, None)
    return lib.qs_pages_fork(*state, a["refs"], a["srows"], a["len"], a["fin"], *geom, None)


ENTRIES = {
    "qs_pages_reserve": (COMMON_FAULTS + RESERVE_FAULTS, RESERVE_NOOPS),
    "qs_pages_release": (COMMON_FAULTS + RELEASE_FAULTS, RELEASE_NOOPS),
    "qs_pages_reserve_refs": (COMMON_FAULTS + RESERVE_FAULTS + REFS_FAULTS, RESERVE_NOOPS),
    "qs_pages_hold": (COMMON_FAULTS + HOLD_FAULTS, HOLD_NOOPS),
    "qs_pages_unhold": (COMMON_FAULTS + UNHOLD_FAULTS, UNHOLD_NOOPS),
    "qs_pages_fork": (COMMON_FAULTS + FORK_FAULTS, FORK_NOOPS),
}


def answers(lib):
    """entry -> [[the call's changes, return code, error text ('' for a no-op)], ...]"""
    out = {}
    for entry, (faults, noops) in ENTRIES.items():
        rows = []
        for change in faults:
            rc = _call(lib, entry, dict(BASE, **change))
            assert rc == -1, f"{entry}{change}: rc {rc} - the call got past the argument checks"
            rows.append([" ".join(f"{k}={v}" for k, v in change.items()), rc, lib.qs_last_error().decode()])
        for change in noops:
            rc = _call(lib, entry, dict(BASE, **change))
            rows.append([" ".join(f"{k}={v}" for k, v in change.items()), rc, ""])
        out[entry] = rows
    return out


def test_every_entry_answers_as_recorded(built_lib):
    from qserve_amd._lib import lib
    with open(GOLDEN) as f:
        golden = json.load(f)
    now = answers(lib)
    assert list(now) == list(golden)
    for entry, rows in now.items():
        assert len(rows) == len(golden[entry]) >= 40, entry
        for got, want in zip(rows, golden[entry]):
            assert got == want, f"{entry}({want[0]}): recorded {want[1:]}, now {got[1:]}"
        assert all(rc == 0 for _, rc, text in rows if text == ""), entry


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from qserve_amd._lib import lib as _lib
    with open(GOLDEN, "w") as g:
        json.dump(answers(_lib), g, indent=0)
        g.write("\n")
