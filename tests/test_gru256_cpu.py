"""GRUModel(gru_size=256), the model `medaka train` builds without a model file (reference models.py DEFAULT_MODEL_DICT), inside
the engine's envelope: `integration._gru_supported` and `engine.pass_plan` (no device needed), and the float64 yardstick on the
live reference's default model where the reference tree is present."""
import numpy as np
import pytest
import torch

from medaka_amd import engine, integration
from oracle import oracle, ref_shim
import ref_standins


@pytest.mark.parametrize("bi", [False, True])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_gru256_is_supported(L, bi):
    for F in range(1, 17):
        assert integration._gru_supported(ref_standins.GRUModel(num_features=F, gru_size=256, n_layers=L, bidirectional=bi))
    assert not integration._gru_supported(ref_standins.GRUModel(num_features=17, gru_size=256, n_layers=L, bidirectional=bi))


@pytest.mark.parametrize("H", [64, 192, 512])
def test_other_widths_stay_outside(H):
    for L, bi in ((1, False), (2, True)):
        assert not integration._gru_supported(ref_standins.GRUModel(gru_size=H, n_layers=L, bidirectional=bi))


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("B", [1, 8, 200, 600, 2000])
def test_pass_plan_is_sequential_and_unfused(B, half):
    for L, bi in ((1, False), (2, True), (4, True)):
        p = engine.pass_plan(B, 10000, num_layers=L, bidirectional=bi, half=half, gru_size=256, host_in=True, host_out=True)
        assert p["windows_per_group"] == (16 if half else 8), p
        assert not any(p[k] for k in ("fuse_layer0", "fuse_projection", "fuse_head", "final_head", "overlap_gemm", "stream_in",
                                      "stream_out")), p
        assert p["needs_gi"], p
        # clusters of 8 CUs, both directions, never more than 224 CUs; gpu_share divides the budget
        assert p["work_groups"] % 8 == 0 and 8 <= p["work_groups"] <= 224, p
        p4 = engine.pass_plan(B, 10000, num_layers=L, bidirectional=bi, half=half, gru_size=256, gpu_share=4)
        assert p4["work_groups"] * 4 <= 224, p4
    # the default keeps today's 128-wide plan
    assert engine.pass_plan(B, 10000, half=half) == engine.pass_plan(B, 10000, half=half, gru_size=128)


@pytest.mark.parametrize("H", [64, 192, 512])
def test_pass_plan_refuses_other_widths(H):
    with pytest.raises(RuntimeError):
        engine.pass_plan(200, 10000, gru_size=H)


@pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")
def test_reference_default_model_is_covered():
    ref_shim.install()
    import medaka.models as ref_models
    torch.manual_seed(3)
    m = ref_models.model_from_dict(ref_models.DEFAULT_MODEL_DICT)
    assert m.gru_size == 256 and integration._gru_supported(m)
    state = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    x = np.random.default_rng(3).random((2, 300, 10), dtype=np.float32)
    with torch.inference_mode():
        want = m(torch.from_numpy(x)).numpy()       # the reference's forward: GRU -> Linear -> softmax (gru.py)
    got = oracle.f64_gru_forward(x, state, n_layers=2, bidirectional=True)
    assert float(np.abs(got - want).max()) <= 1e-5
