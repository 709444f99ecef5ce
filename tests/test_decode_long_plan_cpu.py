"""plan_decode_long (qserve_amd/csrc/attn_plan.h) through its plan-only entry, without a GPU: monotone, inside the split-KV workspace,
and beside - not in place of - the decode dispatcher's plan."""
import pytest

from qserve_amd.long_decode import page_ranges
from qserve_amd.plan import attention_long_plan, attention_plan

CAP = 32 << 20                                 # the split-KV workspace
BATCHES = [1, 2, 3, 8, 63, 64, 65, 255, 256, 512, 1024]
TABLES = [1, 2, 3, 8, 192, 193, 520, 2048, 32768]
HEADS = [(32, 8), (8, 2), (8, 1), (5, 1), (8, 8)]


@pytest.mark.parametrize("int4", [True, False])
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_plan_is_monotone_and_fits(built_lib, H, Hkv, int4):
    for mb in TABLES:
        last = None
        for batch in BATCHES:
            p = attention_long_plan(batch, H, Hkv, mb, int4)
            s = p["splits"]
            assert 1 <= s <= 64 and p["waves"] == 4 and p["min_pages"] >= 1, (batch, mb, p)
            assert s == 1 or s * p["min_pages"] <= mb, (batch, mb, p)                       # never below min_pages pages per range
            assert s == 1 or s * batch * H * 130 * 4 <= CAP, (batch, mb, p)                 # records of O[128], m, l per head and range
            assert batch * Hkv < 512 or s == 1, (batch, mb, p)
            assert last is None or s <= last, f"more sequences, more splits: batch {batch} mb {mb}"
            last = s
    for batch in BATCHES:
        row = [attention_long_plan(batch, H, Hkv, mb, int4)["splits"] for mb in TABLES]
        assert row == sorted(row), f"a longer table, fewer splits: batch {batch} {row}"


def test_one_sequence_fills_the_chip_and_the_dispatcher_stays(built_lib):
    assert attention_long_plan(1, 32, 8, 2048) == dict(splits=32, waves=4, min_pages=2)        # the cap, not 512 / 8
    assert attention_long_plan(8, 32, 8, 2048)["splits"] == 8 and attention_long_plan(8, 32, 8, 2048, False)["splits"] == 4
    assert attention_long_plan(64, 32, 8, 2048)["splits"] == 1
    assert attention_long_plan(0, 32, 8, 2048) == dict(splits=0, waves=0, min_pages=0)
    assert attention_plan(4, 32, 8, 193, 12000)["family"] == "valu"


@pytest.mark.parametrize("length,splits,want", [(1, 64, [(0, 0)]), (64, 3, [(0, 63)]), (201, 3, [(0, 128), (128, 200)]),
                                                (201, 1, [(0, 200)]), (12289, 64, None)])
def test_page_ranges_cover_the_past_once(length, splits, want):
    r = page_ranges(length, splits, 2)
    assert want is None or r == want
    assert r[0][0] == 0 and r[-1][1] == length - 1 and all(a[1] == b[0] for a, b in zip(r, r[1:])) and len(r) <= splits
