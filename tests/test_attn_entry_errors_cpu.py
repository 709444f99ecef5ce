"""The argument checks of the six attention entries, pinned without a GPU: qs_single_query_attention, qs_single_query_attention_quant,
qs_append_attention, qs_append_attention_split, qs_append_tree_attention and qs_append_attention_shared.

Every call below breaks the contract in one place (about twenty per entry) or in two (half a dozen: the FIRST broken check must answer,
so the order of the checks is pinned too) or asks for nothing (a no-op), and returns before any device call - the pointers are small
integers nobody may follow (tests/test_append_split_cpu.py: test_split_entry_validates_before_any_device_call).
tests/golden/attn_entry_errors.json holds each call's return code and the exact qs_last_error() text as the library gave them before
its launchers took argument records.  A deliberate change of a message re-records it:

    python tests/test_attn_entry_errors_cpu.py
"""
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_entry_errors.json")

DECODE = dict(q=16, k=32, v=48, kvp=8, len=8, out=64, qout=80, qsum=96, qscale=112, B=1, H=8, Hkv=2, dh=128, qs=8 * 128, kvs=2 * 128, mb=4,
              mms=256, tpb=64, spt=2 * 64, ts=100, rd=128, base=1e4, neox=1, int4=1, zeros=1)
G9 = dict(H=72, Hkv=8, qs=72 * 128, kvs=8 * 128, spt=8 * 64)          # nine query heads per KV head, everything else in order
DECODE_FAULTS = [dict(q=0), dict(k=0), dict(v=0), dict(kvp=0), dict(out=0), dict(B=-1), dict(H=0), dict(Hkv=0), dict(Hkv=3), dict(dh=64),
                 dict(rd=64), dict(tpb=32), dict(zeros=0), dict(spt=2 * 128), dict(int4=0), dict(mb=0), dict(mms=0), dict(qs=8 * 128 + 4),
                 dict(kvs=2 * 128 - 4), dict(qs=4 * 128), dict(kvs=128), dict(q=8), dict(out=72), dict(v=52), G9,
                 # two faults: the earlier check answers
                 dict(q=0, H=0), dict(Hkv=3, dh=64), dict(dh=64, spt=2 * 128), dict(spt=2 * 128, mb=0), dict(mb=0, qs=8 * 128 + 4),
                 dict(qs=8 * 128 + 4, q=8), dict(G9, q=8), dict(G9, mms=0)]
DECODE_NOOPS = [dict(B=0), dict(B=0, len=0)]
QUANT_FAULTS = [dict(qout=0), dict(qscale=0), dict(qout=0, q=0), dict(qscale=0, Hkv=3), dict(qsum=0, q=0), dict(qsum=0, dh=64)]
QUANT_NOOPS = [dict(B=0, qsum=0)]

APPEND = dict(qkv=16, out=32, cu=1, past=1, kvp=1, mask=8, go=1, pl=1, sg=1, T=4, B=2, NG=1, msq=4, mgt=4, mb=2, H=8, Hkv=2, dh=128, qs=12 * 128,
              os=8 * 128, tpb=64, spt=2 * 64, int4=1, zeros=1, max_past=128, splits=2, mp=64, ms=64, P=1, S=1)
A9 = dict(H=18, Hkv=2, qs=22 * 128, os=18 * 128)                       # nine query heads per KV head
APPEND_FAULTS = [dict(qkv=0), dict(out=0), dict(cu=0), dict(past=0), dict(kvp=0), dict(T=-1), dict(B=-1), dict(msq=-1), dict(mb=0), dict(H=0),
                 dict(Hkv=0), dict(Hkv=3), dict(dh=64), dict(tpb=32), dict(zeros=0), dict(spt=2 * 128), dict(int4=0), dict(qs=12 * 128 + 4),
                 dict(qs=11 * 128), dict(qs=1 << 24), dict(os=7 * 128), dict(os=8 * 128 + 4), dict(qkv=8), dict(out=40), A9,
                 dict(qkv=0, T=-1), dict(T=-1, Hkv=3), dict(Hkv=3, dh=64), dict(dh=64, spt=2 * 128), dict(spt=2 * 128, qs=12 * 128 + 4),
                 dict(qs=12 * 128 + 4, qkv=8), dict(A9, qkv=8)]
APPEND_NOOPS = [dict(T=0), dict(B=0, NG=0), dict(msq=0)]
SPLIT_FAULTS = [dict(splits=-1), dict(splits=-1, max_past=-1), dict(splits=-1, qkv=8), dict(A9, splits=-1), dict(A9, max_past=-1)]
TREE_FAULTS = [dict(mask=0), dict(mask=4), dict(msq=65, T=65), dict(splits=-1), dict(mask=0, qkv=8), dict(mask=0, msq=65), dict(mask=4, msq=65),
               dict(msq=65, splits=-1), dict(A9, splits=-1), dict(A9, mask=4)]
SHARED_FAULTS = [dict(go=0), dict(pl=0), dict(sg=0), dict(NG=0), dict(NG=3), dict(NG=-1), dict(mgt=-1), dict(P=-2), dict(S=-1),
                 dict(go=0, qkv=8), dict(go=0, NG=0), dict(NG=0, P=-2), dict(P=-2, S=-1), dict(A9, P=-2), dict(A9, NG=3), dict(P=-2, mp=-1, ms=-1)]
SHARED_NOOPS = [dict(mgt=0), dict(T=0, P=-1, S=0, mp=-1, ms=-1)]


def _decode(lib, quant, a):
    head = (a["q"], a["k"], a["v"], a["kvp"], a["len"], a["out"])
    tail = (a["B"], a["H"], a["Hkv"], a["dh"], a["qs"], a["kvs"], a["mb"], a["mms"], a["tpb"], a["spt"], a["ts"], a["rd"], a["base"], a["neox"],
            a["int4"], a["zeros"], None)
    if quant:
        return lib.qs_single_query_attention_quant(*head, a["qout"], a["qsum"], a["qscale"], *tail)
    return lib.qs_single_query_attention(*head, *tail)


def _append(lib, entry, a):
    head = (a["qkv"], a["out"], a["cu"], a["past"], a["kvp"])
    mid = (a["mb"], a["H"], a["Hkv"], a["dh"], a["qs"], a["os"], a["tpb"], a["spt"], a["int4"], a["zeros"])
    if entry == "qs_append_attention":
        return lib.qs_append_attention(*head, a["T"], a["B"], a["msq"], *mid, None)
    if entry == "qs_append_attention_split":
        return lib.qs_append_attention_split(*head, a["T"], a["B"], a["msq"], *mid, a["max_past"], a["splits"], None)
    if entry == "qs_append_tree_attention":
        return lib.qs_append_tree_attention(*head, a["mask"], a["T"], a["B"], a["msq"], *mid, a["max_past"], a["splits"], None)
    return lib.qs_append_attention_shared(*head, a["go"], a["pl"], a["sg"], a["T"], a["B"], a["NG"], a["msq"], a["mgt"], *mid, a["mp"], a["ms"],
                                          a["P"], a["S"], None)


ENTRIES = {
    "qs_single_query_attention": (DECODE, DECODE_FAULTS, DECODE_NOOPS, lambda lib, a: _decode(lib, False, a)),
    "qs_single_query_attention_quant": (DECODE, DECODE_FAULTS + QUANT_FAULTS, DECODE_NOOPS + QUANT_NOOPS, lambda lib, a: _decode(lib, True, a)),
    "qs_append_attention": (APPEND, APPEND_FAULTS, APPEND_NOOPS, lambda lib, a: _append(lib, "qs_append_attention", a)),
    "qs_append_attention_split": (APPEND, APPEND_FAULTS + SPLIT_FAULTS, APPEND_NOOPS,
                                  lambda lib, a: _append(lib, "qs_append_attention_split", a)),
    "qs_append_tree_attention": (APPEND, APPEND_FAULTS + TREE_FAULTS, APPEND_NOOPS, lambda lib, a: _append(lib, "qs_append_tree_attention", a)),
    "qs_append_attention_shared": (APPEND, APPEND_FAULTS + SHARED_FAULTS, APPEND_NOOPS + SHARED_NOOPS,
                                   lambda lib, a: _append(lib, "qs_append_attention_shared", a)),
}


def answers(lib):
    """entry -> [[the call's changes, return code, error text ('' for a no-op)], ...]"""
    out = {}
    for entry, (base, faults, noops, call) in ENTRIES.items():
        rows = []
        for change in faults:
            rc = call(lib, dict(base, **change))
            assert rc in (-1, -2), f"{entry}{change}: rc {rc} - the call got past the argument checks"
            rows.append([" ".join(f"{k}={v}" for k, v in change.items()), rc, lib.qs_last_error().decode()])
        for change in noops:
            rc = call(lib, dict(base, **change))
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
        assert len(rows) == len(golden[entry]) >= 26, entry
        for got, want in zip(rows, golden[entry]):
            assert got == want, f"{entry}({want[0]}): recorded {want[1:]}, now {got[1:]}"
        assert all(rc == 0 for _, rc, text in rows if text == ""), entry


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from qserve_amd._lib import lib as _lib
    with open(GOLDEN, "w") as g:
        json.dump(answers(_lib), g, indent=0)
        g.write("\n")
