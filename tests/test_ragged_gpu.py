"""Ragged calls on the device (-m gpu): windows of their own lengths in one forward (include/medaka_amd.h
`mdk_gru_forward_ragged`).

The contract: the probabilities a ragged call returns for window i are, BIT FOR BIT, what `forward_host(x_i[None])` returns for
that window alone on the sequential scan (conftest.py pins MDK_SCAN_SPLIT=0) -- whatever shares the call, in whatever order,
however the engine tiles it, whatever an earlier call left in the workspace.  Against float64 (`oracle.f64_gru_forward`, per
window) the project's tolerances hold: fp32 parity 2e-5, half precision 2e-3, with `test_parity_gpu._check`'s argmax rule."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import weight_set
from medaka_amd import engine, integration, lib, models, synth
from medaka_amd.torch_ext import Batch
from oracle import oracle
from oracle import stitch_oracle as so
from test_parity_gpu import _check

pytestmark = pytest.mark.gpu
TOL, TOL_HALF = 2e-5, 2e-3
MIXED = [1, 2, 7, 8, 9, 17, 33, 600, 5, 601, 13]      # 11 windows: a partly filled second tile, odd longest window
RESUME = [4096, 4095, 2049, 100, 1]                   # longest window 4096: the side-stream overlap and its resumable launches


def _windows(lengths, F=10, seed=0, scale=1.0):
    return [oracle.arch_input(synth.counts_windows(1, n, depth=40, seed=seed + 31 * i + n), F, seed=seed + i)[0] * np.float32(scale)
            for i, n in enumerate(lengths)]


def _singles(e, xs):
    return [e.forward_host(x[None])[0] for x in xs]


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: window {i} ({len(w)} columns) differs from its single-window call"


def _vs_f64(got, refs, half, what, strict=False):
    err = max(float(np.abs(g - r).max()) for g, r in zip(got, refs))
    print(f"{what} {'half' if half else 'fp32'}: max|dp| against float64 = {err:.2e}")
    for i, (g, r) in enumerate(zip(got, refs)):
        _check(g, r, tol=TOL_HALF if half else TOL, what=f"{what} window {i} half={half}", strict_argmax=strict)


@pytest.fixture(scope="module")
def trained(gold):
    """The trained model's state, the two window lists, their float64 references (computed once) and, per precision, the
    single-window calls of a fresh engine."""
    st = weight_set(gold, "trained")
    data = {"state": st, "mixed": _windows(MIXED, seed=11), "resume": _windows(RESUME, seed=12)}
    data["mixed_f64"] = [oracle.f64_gru_forward(x[None], st)[0] for x in data["mixed"]]
    e = engine.GruEngine(st)
    for half in (False, True):
        e.set_precision(half)
        data["mixed", half] = _singles(e, data["mixed"])
        data["resume", half] = _singles(e, data["resume"])
    e.close()
    return data


# ---- mixed lengths inside and across tiles ---------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_mixed_lengths_any_tile_any_order(trained, half):
    xs, want = trained["mixed"], trained["mixed", half]
    e = engine.GruEngine(trained["state"])
    e.set_precision(half)
    for tile in ((0, 4, 8, 16) if half else (0, 4, 8)):
        e.set_option("rec_windows_per_tile", tile)
        got = e.forward_ragged_host(xs)
        _same(got, want, f"tile {tile}")
        assert e.split()["status"] == "not used"
    e.set_option("rec_windows_per_tile", 0)
    _vs_f64(got, trained["mixed_f64"], half, "mixed lengths", strict=not half)
    n = len(xs)
    for order in (list(range(n))[::-1], np.random.default_rng(4).permutation(n).tolist(), [7, 0], [9]):
        _same(e.forward_ragged_host([xs[i] for i in order]), [want[i] for i in order], f"order {order}")
    e.close()


# ---- the resume path under the mask ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_resumed_launches_under_the_mask(trained, half):
    plan = engine.pass_plan(len(RESUME), max(RESUME), half=half, ragged=True)
    assert plan["overlap_gemm"] and not plan["fuse_projection"], plan
    xs, want = trained["resume"], trained["resume", half]
    e = engine.GruEngine(trained["state"])
    e.set_precision(half)
    e.enable_timing(True)
    _same(e.forward_ragged_host(xs), want, "overlap_gemm 1")
    assert e.timing()["rec_launches"] > 2, e.timing()          # (the layers were cut into resumable launches)
    e.set_option("overlap_gemm", 0)
    _same(e.forward_ragged_host(xs), want, "overlap_gemm 0")
    assert e.timing()["rec_launches"] == 2, e.timing()
    e.close()


# ---- a dirty workspace ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_dirty_workspace(trained, half):
    """A rectangular 16 x 4096 forward on other data first: every buffer a ragged call pads into holds that call's values."""
    e = engine.GruEngine(trained["state"])
    e.set_precision(half)
    e.forward_host(synth.counts_windows(16, 4096, depth=40, seed=99))
    _same(e.forward_ragged_host(trained["mixed"]), trained["mixed", half], "mixed after 16 x 4096")
    _same(e.forward_ragged_host(trained["resume"]), trained["resume", half], "resume after 16 x 4096")
    _same(e.forward_ragged_host(trained["mixed"]), trained["mixed", half], "mixed after resume")
    e.close()


# ---- every kind of architecture ----------------------------------------------------------------------------------------------
ARCHS = [(7, 1, True), (16, 2, True), (10, 3, True), (16, 4, False), (7, 2, False)]


@pytest.mark.parametrize("F,L,bi", ARCHS, ids=[f"F{F}-L{L}{'bi' if bi else 'uni'}" for F, L, bi in ARCHS])
def test_architecture_grid(F, L, bi):
    st = oracle.arch_state(F, L, bi)
    xs = _windows([3, 17, 600, 64, 255], F=F, seed=100 * F + L)
    refs = [oracle.f64_gru_forward(x[None], st, n_layers=L, bidirectional=bi)[0] for x in xs]
    assert engine.pass_plan(5, 600, num_features=F, num_layers=L, bidirectional=bi, ragged=True)["fuse_layer0"] == (F < 16)
    e = engine.GruEngine(st, num_features=F, n_layers=L, bidirectional=bi)
    for half in (False, True):
        e.set_precision(half)
        want = _singles(e, xs)
        got = e.forward_ragged_host(xs)
        _same(got, want, f"F={F} L={L} bi={bi} half={half}")
        _vs_f64(got, refs, half, f"arch F={F} L={L} {'bi' if bi else 'uni'}")
    e.close()


# ---- input beyond fp16 range: the on-device fallback twin ----------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_beyond_fp16_range(trained, half):
    xs = [x * np.float32(3000.0) for x in trained["mixed"]]
    refs = [oracle.f64_gru_forward(x[None], trained["state"])[0] for x in xs]
    e = engine.GruEngine(trained["state"])
    e.set_precision(half)
    e.enable_timing(True)
    got = e.forward_ragged_host(xs)                     # (first: the decision is the device's, nothing on the host has seen the flag)
    assert e.timing()["fused_layers"] & (1 << 10), "the range flag is up: layer 0 ran its unfused twin (rec_mfma.hpp, MDK_PF - 1, RAG)"
    _same(got, _singles(e, xs), "un-normalised counts")
    _same(e.forward_ragged_host(xs), got, "again")
    for tile in ((4, 8, 16) if half else (4, 8)):       # every fallback twin
        e.set_option("rec_windows_per_tile", tile)
        _same(e.forward_ragged_host(xs), got, f"tile {tile}")
        assert e.timing()["fused_layers"] & (1 << 10)
    e.set_option("rec_windows_per_tile", 0)
    _vs_f64(got, refs, half, "beyond fp16 range")
    # and in-range input afterwards
    _same(e.forward_ragged_host(trained["mixed"]), trained["mixed", half], "in range afterwards")
    assert not e.timing()["fused_layers"] & (1 << 10)
    e.close()


# ---- the exact kernels -----------------------------------------------------------------------------------------------------------
def test_exact_variant(trained):
    xs = trained["mixed"]
    e = engine.GruEngine(trained["state"])
    e.set_variant(lib.MDK_VARIANT_EXACT)
    got = e.forward_ragged_host(xs)
    _same(got, _singles(e, xs), "MDK_VARIANT_EXACT")
    _same(e.forward_ragged_host(xs[::-1]), got[::-1], "MDK_VARIANT_EXACT reversed")
    err = max(float(np.abs(g - w).max()) for g, w in zip(got, trained["mixed", False]))
    print(f"exact vs MFMA kernels on the mixed list: max|dp| = {err:.2e}")
    assert err <= 2e-5
    e.close()


# ---- equal lengths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_equal_lengths_are_the_rectangular_call(trained, half):
    x = synth.counts_windows(9, 600, depth=40, seed=21)
    e = engine.GruEngine(trained["state"])
    e.set_precision(half)
    want = e.forward_host(x)
    got = e.forward_ragged_host(list(x))
    assert np.array_equal(np.stack(got), want)
    e.close()


# ---- the device entry ----------------------------------------------------------------------------------------------------------
def test_device_entry_on_a_side_stream(trained):
    xs, want = trained["mixed"], trained["mixed", False]
    e = engine.GruEngine(trained["state"])
    lengths = [len(x) for x in xs]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xd = torch.from_numpy(np.concatenate(xs)).cuda()
        yd = torch.full((sum(lengths), 5), -1.0, dtype=torch.float32, device="cuda")
        e.forward_ragged_ptr(xd.data_ptr(), lengths, yd.data_ptr(), stream=stream.cuda_stream)
        e.forward_ragged_ptr(xd.data_ptr(), lengths, yd.data_ptr(), stream=stream.cuda_stream)     # (back to back: the lengths' staging is reused)
    stream.synchronize()
    out = yd.cpu().numpy()
    ends = np.cumsum(lengths)
    _same([out[b - n:b] for b, n in zip(ends, lengths)], want, "device entry")
    e.close()


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_engine_usable(trained):
    e = engine.GruEngine(trained["state"])
    x = synth.counts_windows(3, 40, depth=40, seed=5)
    want = e.forward_host(x)
    with pytest.raises(lib.EngineError, match="bad argument.*length 0"):
        e.forward_ragged_host([x[0], x[1][:0], x[2]])
    buf = np.zeros(8, np.float32)
    L = lib.load()
    no_lengths = ctypes.POINTER(ctypes.c_int)()
    assert L.mdk_gru_forward_ragged(e._h, buf.ctypes.data, no_lengths, 0, buf.ctypes.data) == lib.MDK_OK          # B = 0: a no-op
    assert L.mdk_gru_forward_ragged_dev(e._h, None, no_lengths, 0, None, None) == lib.MDK_OK
    assert e.timing()["gi_ms"] == [0.0, 0.0], "n_layers is filled for an empty call too"
    one = (ctypes.c_int * 1)(1)
    assert L.mdk_gru_forward_ragged(e._h, buf.ctypes.data, one, -1, buf.ctypes.data) == lib.MDK_ERR_ARG
    assert L.mdk_gru_forward_ragged(e._h, None, one, 1, buf.ctypes.data) == lib.MDK_ERR_ARG and "null buffer" in lib.last_error()
    assert L.mdk_gru_forward_ragged(e._h, buf.ctypes.data, no_lengths, 1, buf.ctypes.data) == lib.MDK_ERR_ARG
    e.set_option("max_rows_per_pass", 64)               # 8 x 40 columns of padded area do not fit 64
    with pytest.raises(lib.EngineError, match="column budget"):
        e.forward_ragged_host(list(x))
    e.set_option("max_rows_per_pass", 0)
    assert np.array_equal(e.forward_host(x), want), "the next rectangular call"
    assert np.array_equal(np.stack(e.forward_ragged_host(list(x))), want)
    e.close()
    from test_gru256_gpu import state256
    wide = engine.GruEngine(state256(10, 1, True), gru_size=256, n_layers=1)
    with pytest.raises(lib.EngineError, match="bad argument.*gru_size 256"):
        wide.forward_ragged_host(list(x))
    wide.close()


# ---- the model API ----------------------------------------------------------------------------------------------------------------
def _model(state, **kw):
    m = models.GRUModel(**kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return m.to("cuda").eval()


def test_model_predict_on_ragged(trained, monkeypatch):
    xs = trained["mixed"]
    m = _model(trained["state"])
    spy = []
    eng = m.engine()
    orig = eng.forward_ragged_host
    eng.forward_ragged_host = lambda ws: spy.append(len(ws)) or orig(ws)
    out = m.predict_on_ragged([torch.from_numpy(x) if i % 2 else x for i, x in enumerate(xs)])
    assert spy == [len(xs)]
    assert all(isinstance(p, torch.Tensor) and p.dtype == torch.float32 and p.device.type == "cpu" for p in out)
    _same([p.numpy() for p in out], trained["mixed", False], "predict_on_ragged (input order)")
    one = m.predict_on_batch(Batch(counts_matrix=torch.from_numpy(xs[7])[None])).numpy()[0]
    assert np.array_equal(out[7].numpy(), one)
    # more windows than one call may pad: small calls forced through max_cols, every window still comes back, in input order
    del spy[:]
    out = m.predict_on_ragged(xs, max_cols=1024)
    assert len(spy) >= 3 and sum(spy) == len(xs), spy
    _same([p.numpy() for p in out], trained["mixed", False], "predict_on_ragged, several calls")
    assert m.predict_on_ragged([]) == []
    # a window too long for a ragged call (its tile of 8 beyond the pass's column budget) takes the rectangular entry
    del spy[:]
    monkeypatch.setattr(models, "_RAGGED_PASS_COLUMNS", 8 * 600)
    out = m.predict_on_ragged(xs)
    assert spy == [len(xs) - 1], spy
    _same([p.numpy() for p in out], trained["mixed", False], "predict_on_ragged, one window through predict_on_batch's path")
    monkeypatch.undo()
    single = lambda x: m.predict_on_batch(Batch(counts_matrix=torch.from_numpy(x)[None])).numpy()[0]
    m.exact_kernels = True
    ex = [p.numpy() for p in m.predict_on_ragged(xs[:4])]
    _same(ex, [single(x) for x in xs[:4]], "predict_on_ragged with exact_kernels")
    assert max(float(np.abs(a - b).max()) for a, b in zip(ex, trained["mixed", False])) <= 2e-5
    assert not all(np.array_equal(a, b) for a, b in zip(ex, trained["mixed", False])), "exact_kernels is honoured"
    m.exact_kernels = False
    # half() rounds the parameters themselves to fp16 (the reference's `model.half()`): the yardstick is this model's own
    # single-window call, which runs the half-precision kernels
    m.half()
    got = [p.numpy() for p in m.predict_on_ragged(xs)]
    _same(got, [single(x) for x in xs], "predict_on_ragged after half()")
    assert not all(np.array_equal(a, b) for a, b in zip(got, trained["mixed", False])), "half() is honoured"
    m.normalise = False
    logits = [p.numpy() for p in m.predict_on_ragged(xs[:4])]
    _same(logits, [single(x) for x in xs[:4]], "predict_on_ragged with normalise off")
    assert abs(float(logits[3].sum(-1)[0]) - 1.0) > 1e-3, "normalise is honoured"


def test_model_predict_on_ragged_gru256():
    from test_gru256_gpu import state256
    st = state256(10, 2, True)
    m = _model(st, gru_size=256)
    xs = _windows([5, 40, 13], seed=3)
    out = m.predict_on_ragged(xs)
    for x, p in zip(xs, out):
        assert p.dtype == torch.float32 and p.device.type == "cpu"
        assert np.array_equal(p.numpy(), m.predict_on_batch(Batch(counts_matrix=torch.from_numpy(x)[None])).numpy()[0])


# ---- the loop -------------------------------------------------------------------------------------------------------------------
class _Spy:
    def __init__(self, model):
        self.model, self.batches, self.ragged = model, [], []
        self.half_precision, self.bidirectional = model.half_precision, model.bidirectional

    def predict_on_batch(self, batch):
        self.batches.append(tuple(batch.counts_matrix.shape))
        return self.model.predict_on_batch(batch)

    def predict_on_ragged(self, windows):
        self.ragged.append(len(windows))
        return self.model.predict_on_ragged(windows)


def test_remainder_pass_of_the_loop(trained, monkeypatch):
    """`so.predict` (the restated prediction.py:84-222): one contig of 3 000 columns in chunks of 1 000, then 40 short contigs as
    the remainder pass -- once as the reference runs it (one window per call), once through `integration.predict_remainders`."""
    chunk_len, ovlp = 1000, 200
    rng = np.random.default_rng(17)
    srcs = {}
    for name, cols in [("big", 3000)] + [(f"short{i:02d}", int(n)) for i, n in enumerate(rng.integers(1, 1000, 40))]:
        raw = synth.counts_windows(1, cols, depth=50, seed=1000 + cols, raw=True)
        feats = (raw["counts"][0] / np.maximum(1, raw["depth"][0])[:, None]).astype(np.float32)
        srcs[name] = [so.Pileup(name, feats, so.make_positions(raw["major"][0], raw["minor"][0]), None, raw["depth"][0])]
    model = _model(trained["state"])

    def run(spy):
        return so.predict(so.contig_regions(srcs), lambda r: so.pileups_in_region(srcs, r), spy, Batch.collate, chunk_len, ovlp, 200, 10**9)
    plain = _Spy(model)
    want = run(plain)
    assert plain.ragged == [] and sorted(plain.batches)[-1] == (4, 1000, 10) and len(plain.batches) == 41
    orig = so.run_prediction

    def run_prediction(store, regions, pileups_of, mdl, collate, chunk_len, chunk_ovlp, batch_size=200, enable_chunking=True,
                       workers=2, on_batch=None):
        if not (batch_size == 1 and not enable_chunking):
            return orig(store, regions, pileups_of, mdl, collate, chunk_len, chunk_ovlp, batch_size, enable_chunking, workers, on_batch)
        loader = so.Loader(regions, pileups_of, collate, batch_size, chunk_len, chunk_ovlp, enable_chunking, workers)

        def write(sample, probs, feat):
            assert tuple(feat.shape) == sample.features.shape
            if sample.name not in store:
                store[sample.name] = sample.with_probs(np.array(probs.numpy()))
        integration.predict_remainders(loader, mdl, write)
        return loader.remainders
    monkeypatch.setattr(so, "run_prediction", run_prediction)
    spy = _Spy(model)
    got = run(spy)
    assert spy.batches == [(4, 1000, 10)], "the batched pass is unchanged"
    assert 1 <= len(spy.ragged) <= 2 and sum(spy.ragged) == 40, spy.ragged
    assert sorted(got) == sorted(want) and len(got) == 4 + 40
    for name in want:
        assert np.array_equal(got[name].label_probs, want[name].label_probs), name
    lengths = {r.ref_name: r.end for r in so.contig_regions(srcs)}
    assert so.fastq(got, lengths) == so.fastq(want, lengths)
