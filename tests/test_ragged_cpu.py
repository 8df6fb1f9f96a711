"""Ragged calls without a device: the grouping policy (`engine.ragged_calls`), the plan of a ragged pass
(`engine.pass_plan(..., ragged=True)`) and the hook that routes the remainder pass of the UNMODIFIED reference's
`run_prediction` (prediction.py:14-81, called with batch_size 1 and no chunking from :204-209) through
`integration.predict_remainders`."""
import types

import numpy as np
import pytest
import torch

from medaka_amd import engine, integration
from oracle import ref_shim


# ---- the grouping policy ---------------------------------------------------------------------------------------------------
def _ceil8(n):
    return (n + 7) // 8 * 8


def _check_calls(lengths, calls, cap, max_cols):
    flat = sorted(i for c in calls for i in c)
    assert flat == list(range(len(lengths))), "every index exactly once"
    for c in calls:
        assert c and lengths[c[0]] == max(lengths[i] for i in c), "the first index of a call is its longest window"
        assert len(c) <= cap
        if len(c) > 1:
            assert _ceil8(len(c)) * lengths[c[0]] <= max_cols


@pytest.mark.parametrize("half,bi,share", [(False, True, 1), (True, True, 1), (False, False, 1), (True, False, 2), (False, True, 4)])
def test_ragged_calls_policy(half, bi, share):
    cap = engine.ragged_window_cap(half, bi, share)
    # the cap is the largest count the ragged plan keeps in one round of work-groups at the largest tile
    D = 2 if bi else 1
    plan = engine.pass_plan(cap, 600, bidirectional=bi, half=half, gpu_share=share, ragged=True)
    over = engine.pass_plan(cap + 1, 600, bidirectional=bi, half=half, gpu_share=share, ragged=True)
    assert plan["work_groups"] * D <= 232 // share < over["work_groups"] * D, (plan, over)
    assert plan["windows_per_group"] == (16 if half else 8)
    rng = np.random.default_rng(5)
    for lengths, max_cols in ((rng.integers(1, 10000, 400).tolist(), 1 << 21), (rng.integers(1, 700, 5000).tolist(), 1 << 21),
                              (rng.integers(1, 10000, 300).tolist(), 1 << 16), ([7], 1 << 21), ([5000, 3, 3], 4096)):
        calls = engine.ragged_calls(lengths, half=half, bidirectional=bi, gpu_share=share, max_cols=max_cols)
        _check_calls(lengths, calls, cap, max_cols)


def test_ragged_calls_figures():
    assert engine.ragged_window_cap(False) == 928 and engine.ragged_window_cap(True) == 1856
    assert len(engine.ragged_calls([500] * 2000)) == 3
    assert len(engine.ragged_calls([500] * 2000, half=True)) == 2
    calls = engine.ragged_calls([9999] * 400)
    assert max(len(c) for c in calls) <= 208 and sum(len(c) for c in calls) == 400
    assert engine.ragged_calls([]) == []
    # longest first, stable: equal lengths keep their input order; a window beyond max_cols is a call by itself
    assert engine.ragged_calls([3, 9, 3, 9]) == [[1, 3, 0, 2]]
    assert engine.ragged_calls([10, 5000, 10], max_cols=4096) == [[1], [0, 2]]


# ---- the plan of a ragged pass ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("B,T", [(5, 600), (16, 4096), (928, 2000), (1000, 2000)])
def test_ragged_pass_plan(B, T, half):
    for host in (False, True):
        plan = engine.pass_plan(B, T, half=half, host_in=host, host_out=host, ragged=True)
        for k in ("fuse_projection", "fuse_head", "final_head", "stream_in", "stream_out"):
            assert not plan[k], (k, plan)
        assert plan["needs_gi"], plan
        assert plan["overlap_gemm"] == ((B, T) == (16, 4096)), plan
    # a caller that looks at the range flag itself changes nothing: the decision of a ragged call stays on the device
    assert engine.pass_plan(B, T, half=half, ragged=True, host_checks_range=True)["needs_gi"]


def test_rectangular_pass_plans_are_what_they_were():
    """The same shapes without `ragged`, host entry, both precisions: the values of the library before ragged calls existed."""
    keys = ("windows_per_group", "work_groups", "fuse_layer0", "fuse_projection", "fuse_head", "final_head", "overlap_gemm",
            "stream_in", "stream_out", "needs_gi")
    want = {(5, 600): (4, 2, True, False, False, False, False, False, False, True),
            (16, 4096): (4, 4, True, False, False, False, True, True, True, True),
            (928, 2000): (8, 116, True, True, True, True, False, False, False, True),
            (1000, 2000): (8, 125, True, True, True, True, False, False, False, True)}
    for (B, T), w in want.items():
        for half in (False, True):
            plan = engine.pass_plan(B, T, host_in=True, host_out=True, half=half)
            assert tuple(plan[k] for k in keys) == w, ((B, T), half, plan)
    assert not engine.pass_plan(1000, 2000, host_checks_range=True)["needs_gi"]


# ---- the hook against the unmodified reference ---------------------------------------------------------------------------------
class _Sample:
    """what the reference's loop reads of a `medaka.common.Sample` (prediction.py:47-66)"""
    def __init__(self, name, feats):
        self.name, self.features, self.label_probs = name, feats, None
        self.size = self.span = 0 if feats is None else len(feats)
        self.last_pos = (self.size - 1, 0)

    def _get_pos(self, i):
        return (i, 0)

    def amend(self, **kw):
        new = _Sample(self.name, kw.get("features"))
        new.label_probs = kw["label_probs"]
        return new


class _RaggedModel:
    """probabilities of a window = its own column sums, so that a row handed to the wrong sample shows"""
    def __init__(self):
        self.ragged_calls, self.batch_calls = [], 0

    def predict_on_ragged(self, windows):
        self.ragged_calls.append(len(windows))
        return [torch.as_tensor(np.asarray(w)).float().sum(-1, keepdim=True).repeat(1, 5) for w in windows]

    def predict_on_batch(self, batch):
        self.batch_calls += 1
        return batch.features.float().sum(-1, keepdim=True).repeat(1, 1, 5)


class _BatchModel:
    def __init__(self):
        self.batch_calls = 0

    predict_on_batch = _RaggedModel.predict_on_batch


@pytest.fixture
def ref_loop(monkeypatch):
    """The reference's prediction module with its DataLoader and DataStore replaced by stand-ins: the loader yields
    batch_size-sized (data, batch) pairs of fake samples and exposes `remainders`, the store records what is written."""
    if not ref_shim.available():
        pytest.skip("reference tree not present")
    ref_shim.install()
    import medaka.datastore
    import medaka.prediction
    rng = np.random.default_rng(3)
    samples = [_Sample(f"ctg{i}:0.0-{n}.0", rng.random((n, 10), dtype=np.float32)) for i, n in enumerate((13, 777, 1, 40, 41, 300))]
    made = {}

    class Loader:
        def __init__(self, bam, regions, batch_size, **kw):
            from medaka_amd import torch_ext
            self.batch_size, self.kw, self.remainders = batch_size, kw, [("left-over", 3)]
            self.target_at_init = torch_ext.stage_target()
            made["loader"] = self

        def __iter__(self):
            for i in range(0, len(samples), self.batch_size):
                data = samples[i:i + self.batch_size]
                T = max(s.features.shape[0] for s in data)
                x = np.zeros((len(data), T, 10), dtype=np.float32)
                for k, s in enumerate(data):
                    x[k, :s.features.shape[0]] = s.features
                yield data, types.SimpleNamespace(features=torch.from_numpy(x))

    class Store:
        def __init__(self, path, mode):
            self.path, self.mode, self.written = path, mode, []
            made["store"] = self

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def write_sample(self, sample):
            self.written.append(sample)

    monkeypatch.setattr(medaka.prediction, "DataLoader", Loader)
    monkeypatch.setattr(medaka.datastore, "DataStore", Store)
    regions = [types.SimpleNamespace(size=s.features.shape[0]) for s in samples]
    yield medaka.prediction, samples, regions, made
    integration.uninstall()


def _run(mp, regions, model, **kw):
    return mp.run_prediction("out.hdf", "bam", regions, model, "fenc", 1000, 200, **kw)


def test_hook_routes_the_remainder_pass(ref_loop, monkeypatch):
    mp, samples, regions, made = ref_loop
    monkeypatch.delenv("MEDAKA_AMD_RAGGED", raising=False)
    orig = mp.run_prediction
    integration.install(collate=False)
    assert mp.run_prediction is not orig
    # the early hand-over of batches is off while the ragged loop runs -- from before the loader exists -- and back afterwards
    from medaka_amd import torch_ext
    target = type("Engine", (), {"_h": 1})()                     # (what the hook reads of a GruEngine: an open handle)
    seen = []
    for save in (False, True):
        torch_ext.set_stage_target(target)
        model = _RaggedModel()
        model.predict_on_ragged = (lambda ws, f=model.predict_on_ragged: seen.append(torch_ext.stage_target()) or f(ws))
        left = _run(mp, regions, model, batch_size=1, save_features=save, enable_chunking=False)
        assert left == [("left-over", 3)] and left is made["loader"].remainders
        assert made["loader"].kw["enable_chunking"] is False and made["loader"].batch_size == 1
        assert (made["store"].path, made["store"].mode) == ("out.hdf", "a")
        written = made["store"].written
        assert [w.name for w in written] == [s.name for s in samples], "every sample once"
        for w, s in zip(written, samples):
            assert torch.equal(w.label_probs, torch.from_numpy(s.features).sum(-1, keepdim=True).repeat(1, 5)), "its own row"
            if save:
                assert np.array_equal(np.asarray(w.features), s.features)
            else:
                assert w.features is None
        assert model.batch_calls == 0 and sum(model.ragged_calls) == len(samples)
        assert len(model.ragged_calls) < len(samples), "fewer model calls than samples"
        assert made["loader"].target_at_init is None and seen and all(t is None for t in seen)
        assert torch_ext.stage_target() is target
    torch_ext.set_stage_target(None)
    integration.uninstall()
    assert mp.run_prediction is orig


def test_hook_leaves_every_other_call_to_the_reference(ref_loop, monkeypatch):
    mp, samples, regions, made = ref_loop
    monkeypatch.delenv("MEDAKA_AMD_RAGGED", raising=False)
    integration.install(collate=False)
    # the batched pass: the reference's own loop, one predict_on_batch per batch
    model = _RaggedModel()
    _run(mp, regions, model, batch_size=200)
    assert model.ragged_calls == [] and model.batch_calls == 1 and len(made["store"].written) == len(samples)
    # chunking on at batch_size 1 is not the remainder pass
    model = _RaggedModel()
    _run(mp, regions, model, batch_size=1)
    assert model.ragged_calls == [] and model.batch_calls == len(samples)
    # a model without ragged calls (the reference's own classes, MajorityVoteModel ...)
    model = _BatchModel()
    _run(mp, regions, model, batch_size=1, enable_chunking=False)
    assert model.batch_calls == len(samples) and len(made["store"].written) == len(samples)


def test_hook_can_be_switched_off(ref_loop, monkeypatch):
    mp, samples, regions, made = ref_loop
    orig = mp.run_prediction
    monkeypatch.setenv("MEDAKA_AMD_RAGGED", "0")
    integration.install(collate=False)
    assert mp.run_prediction is orig
    model = _RaggedModel()
    _run(mp, regions, model, batch_size=1, enable_chunking=False)
    assert model.ragged_calls == [] and model.batch_calls == len(samples)
    integration.uninstall()
    monkeypatch.delenv("MEDAKA_AMD_RAGGED")
    integration.install(collate=False, ragged=False)
    assert mp.run_prediction is orig


def test_predict_remainders_flushes_at_the_cap():
    rng = np.random.default_rng(1)
    samples = [_Sample(str(i), rng.random((n, 10), dtype=np.float32)) for i, n in enumerate((5, 9, 2, 30, 4, 4, 8))]
    batches = [([s], types.SimpleNamespace(features=torch.from_numpy(s.features)[None])) for s in samples]
    for flush_at, want in (((3, 1 << 21), [3, 3, 1]), ((100, 14), [2, 2, 3]), (None, [7])):
        model, got = _RaggedModel(), []
        n = integration.predict_remainders(iter(batches), model, lambda s, p, f: got.append((s.name, p, f)), flush_at=flush_at)
        assert model.ragged_calls == want and n == len(want)
        assert [g[0] for g in got] == [s.name for s in samples]
        for (_, p, f), s in zip(got, samples):
            assert np.array_equal(f.numpy(), s.features) and torch.equal(p[:, 0], torch.from_numpy(s.features).sum(-1))
