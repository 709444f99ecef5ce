"""Per-head Q/K RMSNorm without a GPU: the entry's validation (before any device call), `DecodeEngine` with `qk_norm=True` on the trace
harness of tests/test_engine_trace_cpu.py - one qk_norm_rows per layer and pass, on the qkv rows its consumer reads next -, the loader."""
import pytest
import torch

from test_engine_trace_cpu import PAR, install

A = 0x1000                                     # a made-up, aligned, non-null address: validation comes before any device call
CONSUMERS = ("apply_bias_rope_update_kv_cache ", "append_rope_update_kv_cache ", "append_tree_rope_update_kv_cache ",
             "single_query_attention")         # whatever rotates the qkv rows: the writers and every decode attention family


@pytest.mark.parametrize("args, rc", [
    ((A, A, A, 4, 8, 2, 64, 1536, 1e-6), -2),          # head_dim 64
    ((A, A, A, 4, 8, 2, 128, 1536, 0.0), -1),          # eps = 0
    ((A, A, A, 4, 8, 2, 128, 1528, 1e-6), -1),         # a stride below (H + 2 Hkv) * 128
    ((A, A, 0, 4, 8, 2, 128, 1536, 1e-6), -1),         # a null weight
    ((A, A, A, 0, 8, 2, 128, 1536, 1e-6), 0),          # no tokens: ok, no launch
])
def test_entry_validates_before_any_device_call(built_lib, args, rc):
    from qserve_amd._lib import lib
    assert lib.qs_qk_norm_rows(*args, None) == rc


@pytest.mark.parametrize("entry, passes", [("prefill", 1), ("step", 2), ("prefill_chunked", 3), ("verify_tree", 2)])
def test_engine_norms_each_layers_qkv_rows_in_front_of_their_consumer(built_lib, monkeypatch, entry, passes):
    D, rec = install(monkeypatch)
    eng = rec.watch(D.DecodeEngine(dict(D.TINY, qk_norm=True), 2, 7 if entry == "prefill_chunked" else 5, 4, device="cpu", seed=3))
    eng.prefill_chunked(7, 3) if entry == "prefill_chunked" else eng.prefill(5)      # (chunks of 3, 3 and 1 tokens: three passes)
    if entry == "step":
        eng.step()
    if entry == "verify_tree":
        eng.verify_tree(torch.zeros((2, len(PAR)), dtype=torch.int64), PAR, device_walk=True)
    seq, layers = [ln.split() for ln in rec.lines if ln.startswith(("qk_norm_rows ",) + CONSUMERS)], D.TINY["layers"]
    assert [w[0] == "qk_norm_rows" for w in seq] == [True, False] * (layers * passes), [w[0] for w in seq]
    for i, (norm, consumer) in enumerate(zip(seq[::2], seq[1::2])):
        assert norm[1] == consumer[1] and norm[1] in ("bufs.qkv", "qkv_buf"), (norm, consumer)
        assert norm[2:4] == [f"layers[{i % layers}].q_norm", f"layers[{i % layers}].k_norm"] and norm[5:8] == ["4", "2", "128"], norm


def test_off_launches_no_norm_and_moe_refuses(built_lib, monkeypatch):
    D, rec = install(monkeypatch)
    eng = rec.watch(D.DecodeEngine(D.TINY, 2, 5, 4, device="cpu", seed=3))
    eng.prefill(5)
    eng.step()
    assert "q_norm" not in eng.layers[0] and not [ln for ln in rec.lines if ln.startswith("qk_norm_rows")]
    assert D.QWEN3_8B["qk_norm"] is True and D.QWEN3_8B["hidden"] == D.QWEN3_8B["heads"] * 128
    with pytest.raises(AssertionError, match="qk_norm on a mixture-of-experts config is refused"):
        D.DecodeEngine(dict(D.TINY_MOE, qk_norm=True), 2, 5, 4, device="cpu", seed=3)


def test_loader_and_config_must_agree_about_the_norm_weights(built_lib):
    from test_loader import CFG, make_checkpoint
    from qserve_amd.decode import DecodeEngine
    from qserve_amd.loader import load_llama_w4a8
    plain, on = make_checkpoint(-1), dict(CFG, qk_norm=True)
    qwen = dict(plain, **{f"model.layers.{li}.self_attn.{n}_norm.weight": torch.full((128,), v + li)
                          for li in range(CFG["layers"]) for n, v in (("q", 1.0), ("k", 3.0))})
    eng = DecodeEngine(on, 1, 4, 2, device="cpu", weights=load_llama_w4a8(qwen, on))
    assert [(float(L["q_norm"][0]), float(L["k_norm"][-1]), L["q_norm"].dtype) for L in eng.layers] == \
        [(1.0, 3.0, torch.float16), (2.0, 4.0, torch.float16)]
    for state, cfg in ((qwen, CFG), (plain, on)):
        with pytest.raises(RuntimeError, match=f"qk_norm={cfg is on}"):
            load_llama_w4a8(state, cfg)
