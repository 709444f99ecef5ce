"""DecodeEngine with `qk_norm` on the GPU: the captured step replays what the eager steps compute, and the norm is live."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _finals(qk_norm, captured=False):
    """TINY, prompt 40, four steps -> `final` after the prompt and after every step."""
    from qserve_amd import decode as D
    eng = D.DecodeEngine(dict(D.TINY, qk_norm=True) if qk_norm else D.TINY, batch=2, prompt_len=40, max_new=8, device="cuda:0", seed=3)
    eng.prefill(40)
    out = [eng.final.float().clone()]
    for run in [eng.capture] + [eng.run] * 3 if captured else [eng.step] * 4:      # (capture's warm-up is a real step)
        run()
        out.append(eng.final.float().clone())
    torch.cuda.synchronize()
    return torch.stack(out)


def test_captured_step_replays_the_eager_steps_and_the_norm_is_live(gpu):
    eager = _finals(True)
    assert torch.isfinite(eager).all()
    assert torch.equal(_finals(True, captured=True), eager), "captured run differs from the eager steps"
    assert not torch.equal(_finals(False), eager), "the same seed without qk_norm (every other weight the same) computes the same"
