"""The references for every GRUModel architecture the engine accepts (integration._gru_supported: gru_size 128, 1..16
features, 1..4 layers, either direction).

  * `oracle.f64_gru_forward` (PyTorch in float64) is the yardstick of tests/test_arch_envelope_gpu.py; it is pinned here
    to the goldens of the unmodified reference at the default architecture;
  * the fp32 C oracle agrees with it over the whole envelope to 5e-6;
  * the engine's envelope test itself is pinned at its edges."""
import numpy as np
import pytest

from conftest import weight_set
from medaka_amd import integration, synth
from oracle import oracle
import ref_standins

ARCHS = [(L, bi) for L in (1, 2, 3, 4) for bi in (True, False)]


@pytest.mark.parametrize("F", [1, 2, 7, 10, 15, 16])
@pytest.mark.parametrize("L,bi", ARCHS, ids=[f"L{L}{'bi' if bi else 'uni'}" for L, bi in ARCHS])
def test_c_oracle_matches_float64_over_the_envelope(F, L, bi):
    st = oracle.arch_state(F, L, bi)
    x = oracle.arch_input(synth.counts_windows(3, 41, seed=F * 10 + L), F, seed=F)
    ref = oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi)
    out = oracle.c_gru_forward(x, st, n_layers=L, bidirectional=bi)
    assert ref.dtype == np.float64 and ref.shape == out.shape == (3, 41, 5)
    err = float(np.abs(out - ref).max())
    assert err <= 5e-6, err
    assert np.array_equal(out.argmax(-1), ref.argmax(-1))
    # the generated weights are confident: most columns separate their top two by more than twice the half-precision
    # tolerance of the GPU tests, so their argmax checks cover most of the output
    srt = np.sort(ref, -1)
    assert ((srt[..., -1] - srt[..., -2]) > 4e-3).mean() >= 0.6
    logits = oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi, normalise=False)
    assert np.abs(oracle.c_gru_forward(x, st, n_layers=L, bidirectional=bi, normalise=False) - logits).max() <= 5e-5


def test_float64_reference_matches_reference_goldens(gold):
    for key in sorted(gold["gru_outputs"]):
        wname, cname = key.split("/")
        x = gold["gru_inputs"][cname]
        if x.shape[1] > 2000:
            continue
        ref = gold["gru_outputs"][key]
        out = oracle.f64_gru_forward(x, weight_set(gold, wname))
        assert np.abs(out - ref).max() <= 2e-6, key


@pytest.mark.parametrize("pad", ["zero", "random"])
def test_padded_trained_weights(gold, pad):
    """Trained weights widened to 11..16 features: with zero pad weights (any pad input), or with zero pad inputs (any pad
    weights), the model is the 10-feature one -- exactly so in float64."""
    x10 = synth.counts_windows(2, 64, seed=3)
    ref10 = oracle.f64_gru_forward(x10, gold["weights_trained"])
    for F in range(11, 17):
        st = oracle.padded_state(gold["weights_trained"], F, pad=pad, seed=F)
        assert st["gru.weight_ih_l0"].shape == st["gru.weight_ih_l0_reverse"].shape == (384, F)
        assert np.array_equal(st["gru.weight_ih_l0"][:, :10], gold["weights_trained"]["gru.weight_ih_l0"])
        assert (st["gru.weight_ih_l0"][:, 10:] == 0).all() == (pad == "zero")
        x = oracle.arch_input(x10, F, pad=None if pad == "zero" else 0.0, seed=F)
        assert np.array_equal(x[..., :10], x10)
        out = oracle.f64_gru_forward(x, st)
        assert np.abs(out - ref10).max() <= 1e-12, (F, pad)
        assert np.abs(oracle.c_gru_forward(x, st) - ref10).max() <= 2e-6, (F, pad)


@pytest.mark.parametrize("kw,ok", [
    (dict(num_features=0), False), (dict(num_features=1), True), (dict(num_features=16), True),
    (dict(num_features=17), False), (dict(n_layers=1), True), (dict(n_layers=4), True), (dict(n_layers=5), False),
    (dict(n_layers=4, bidirectional=False), True), (dict(num_features=16, n_layers=1, bidirectional=False), True),
    (dict(gru_size=64), False), (dict(gru_size=128), True)])
def test_gru_supported_at_its_edges(kw, ok):
    assert integration._gru_supported(ref_standins.GRUModel(**kw)) is ok


def test_gru_supported_rejects_zero_layers():
    m = ref_standins.GRUModel()           # (torch.nn.GRU refuses to build one: the attribute is what convert() reads)
    m.n_layers = 0
    assert integration._gru_supported(m) is False
