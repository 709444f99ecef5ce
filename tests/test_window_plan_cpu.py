"""plan_decode_window (csrc/attn_plan.h) through its plan entry, and what the windowed entries refuse before any device call."""
import ctypes as C

import pytest
import torch

from qserve_amd._lib import lib
from qserve_amd.plan import attention_long_plan, attention_window_plan

BATCHES = [1, 2, 8, 63, 64, 65, 512]
TABLES = [1, 3, 66, 193, 2048]
WINDOWS = [1, 64, 65, 4096, 10 ** 6, 2 ** 31 - 1]
FAKE = 0x1000                      # a made-up, 16-byte aligned address: nothing may read it


@pytest.mark.parametrize("int4", [True, False])
@pytest.mark.parametrize("H,Hkv", [(32, 8), (8, 2), (5, 1)])
def test_grid_is_a_function_of_table_and_window(built_lib, H, Hkv, int4):
    for mb in TABLES:
        for W in WINDOWS:
            for batch in BATCHES:
                p = attention_window_plan(batch, H, Hkv, mb, W, int4)
                assert 1 <= p["splits"] <= 32 and p["waves"] == 4 and p["min_pages"] >= 1, (batch, mb, W, p)
                assert p["splits"] == 1 or p["splits"] <= min(mb, W // 64 + 2) // p["min_pages"], (batch, mb, W, p)
                if W // 64 + 2 >= mb:              # the window never bounds the chain: the long plan
                    assert p["splits"] == attention_long_plan(batch, H, Hkv, mb, int4)["splits"], (batch, mb, W, p)
    assert attention_window_plan(0, H, Hkv, 8, 64, int4) == dict(splits=0, waves=0, min_pages=0)
    assert attention_window_plan(1, H, Hkv, 2048, 0, int4) == attention_long_plan(1, H, Hkv, 2048, int4), "window = 0: no window"


def _decode(window, dh=128):
    return lib.qs_single_query_attention_window(*(FAKE,) * 6, 1, 8, 2, dh, 8 * 128, 2 * 128, 8, 512, 64, 2 * 64, 5, dh, 1e4, 1, 1, 1, window, 0, None)


def _append(window, dh=128):
    return lib.qs_append_attention_window(*(FAKE,) * 5, 4, 1, 4, 8, 8, 2, dh, 12 * 128, 8 * 128, 64, 2 * 64, 1, 1, window, None)


def test_refused_before_any_device_call(built_lib):
    buf = (C.c_int * 3)()
    assert _decode(-1) == -1 and b"window=-1" in lib.qs_last_error()
    assert _append(-1) == -1 and b"window=-1" in lib.qs_last_error()
    assert lib.qs_single_query_attention_window_plan(1, 8, 2, 8, -1, 1, C.cast(buf, C.c_void_p)) == -1 and list(buf) == [0, 0, 0]
    assert _decode(64, dh=64) == -2 and _append(64, dh=64) == -2          # QS_ENOSUP: head_dim != 128


def test_window_with_a_tree_mask_or_shared_groups_raises():
    from qserve_amd import append
    t = torch.zeros(1)
    for fn, args in ((append.append_tree, (t,) * 5 + (8, 2, 128, 1e4, True)), (append.append_tree_attention, (t,) * 5 + (8, 2, 128, True)),
                     (append.append_shared, (t,) * 4 + (8, 2, 128, 1e4, True, None)),
                     (append.append_attention_shared, (t,) * 4 + (8, 2, 128, True, None))):
        with pytest.raises(NotImplementedError, match="window=64 together with (a tree mask|shared groups)"):
            fn(*args, window=64)
    with pytest.raises(NotImplementedError, match="window=64 together with num_splits"):
        append.append(t, t, t, t, 8, 2, 128, 1e4, True, num_splits=4, window=64)
