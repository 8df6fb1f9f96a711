"""GRUModel(gru_size=256) -- the model `medaka train` builds by default -- on the cluster recurrence (gru_wide.hpp), against
float64 (`oracle.f64_gru_forward`, which reads the width from the state).

fp32-parity mode: max|dp| <= 1e-4 and the float64 argmax wherever float64 separates its top two by more than twice that, over
L in 1..4 x {uni, bi} x F in {1, 10, 16} and ragged shapes, plus long windows and batches larger than one round of clusters.
Half precision: within twice the deviation of the CPU fp16 emulation (`m.half(); m(x.half())`) on the same inputs.
Every entry computes the same bits; a split request runs the sequential scan and is reported as not split."""
import types

import numpy as np
import pytest
import torch

from medaka_amd import engine, integration, synth
from medaka_amd.torch_ext import Batch
from oracle import oracle
import ref_standins

pytestmark = pytest.mark.gpu
H = 256
TOL = 1e-4
ARCHS = [(L, bi) for L in (1, 2, 3, 4) for bi in (False, True)]
ARCH_IDS = [f"L{L}{'bi' if bi else 'uni'}" for L, bi in ARCHS]
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nGRU(256) worst max|dp| against float64:")
    for k, v in sorted(_WORST.items()):
        print(f"  {k}: {v:.2e}")


def state256(F, L, bi, seed=0, gain=2.5, head_gain=7.0):
    """Seeded GRU(256) weights: PyTorch's uniform +-1/sqrt(256), W_hh x `gain`, a confident head (x `head_gain`)."""
    rng = np.random.default_rng(7919 * seed + 1009 * F + 31 * L + int(bi))
    D, k = 2 if bi else 1, 1.0 / np.sqrt(H)
    st = {}
    for layer in range(L):
        kin = F if layer == 0 else D * H
        for sfx in [""] + (["_reverse"] if bi else []):
            st[f"gru.weight_ih_l{layer}{sfx}"] = rng.uniform(-k, k, (3 * H, kin)).astype(np.float32)
            st[f"gru.weight_hh_l{layer}{sfx}"] = (rng.uniform(-k, k, (3 * H, H)) * gain).astype(np.float32)
            st[f"gru.bias_ih_l{layer}{sfx}"] = rng.uniform(-k, k, 3 * H).astype(np.float32)
            st[f"gru.bias_hh_l{layer}{sfx}"] = rng.uniform(-k, k, 3 * H).astype(np.float32)
    st["linear.weight"] = (rng.uniform(-k, k, (5, D * H)) * head_gain).astype(np.float32)
    st["linear.bias"] = rng.uniform(-k, k, 5).astype(np.float32)
    return st


def _engine(st, F, L, bi, **kw):
    return engine.GruEngine(st, num_features=F, gru_size=H, n_layers=L, bidirectional=bi, **kw)


def _x(B, T, F, seed):
    return oracle.arch_input(synth.counts_windows(B, T, depth=40, seed=seed), F, seed=seed)


def _vs_f64(out, ref, key, tol=TOL):
    assert out.shape == ref.shape and np.isfinite(out).all(), key
    err = float(np.abs(out - ref).max()) if out.size else 0.0
    _WORST[key] = max(_WORST.get(key, 0.0), err)
    assert err <= tol, f"{key}: max|dp| = {err:.3e}"
    srt = np.sort(ref, -1)
    clear = (srt[..., -1] - srt[..., -2]) > 2 * tol
    assert (out.argmax(-1) == ref.argmax(-1))[clear].all(), key
    return err


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _forward_dev(e, x, entry="ptr"):
    B, T, _ = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.empty((B, T, 5), dtype=torch.float32, device="cuda")
    (e.forward_ptr if entry == "ptr" else e.forward_async_ptr)(xd.data_ptr(), B, T, yd.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def _torch_model(st, F, L, bi):
    gru = torch.nn.GRU(F, H, num_layers=L, bidirectional=bi, batch_first=True)
    lin = torch.nn.Linear((2 if bi else 1) * H, 5)
    gru.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in st.items() if k.startswith("gru.")})
    lin.load_state_dict({k[7:]: torch.from_numpy(v) for k, v in st.items() if k.startswith("linear.")})
    return gru, lin


def _cpu_half_emulation(st, F, L, bi, x):
    """What `m.half(); m(x.half()).float()` computes on the CPU: the yardstick of half precision."""
    gru, lin = _torch_model(st, F, L, bi)
    with torch.inference_mode():
        gru, lin = gru.half(), lin.half()
        y = torch.softmax(lin(gru(torch.from_numpy(x).half())[0]), dim=-1)
    return y.float().numpy()


# ---- the architecture grid, fp32-parity mode --------------------------------------------------------------------------
@pytest.mark.parametrize("L,bi", ARCHS, ids=ARCH_IDS)
@pytest.mark.parametrize("F", [1, 10, 16])
def test_grid_fp32(F, L, bi):
    st = state256(F, L, bi)
    e = _engine(st, F, L, bi)
    for B, T in ((1, 1), (2, 7), (5, 333)):
        x = _x(B, T, F, seed=F + 10 * L + B + T)
        out = e.forward_host(x)
        _vs_f64(out, oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi), f"fp32 F={F} L={L} bi={bi}")
        assert np.array_equal(e.forward_host(x), out), "two calls differ"
    e.close()


@pytest.mark.parametrize("F,L,bi,B,T", [(10, 2, True, 3, 10000), (16, 1, False, 3, 10000), (10, 2, True, 600, 512),
                                        (1, 3, False, 600, 512)])
def test_long_windows_and_large_batches(F, L, bi, B, T):
    """B = 3 x 10 000 columns; 600 windows = 75 groups of 8: more than one round of clusters (two interleaved groups each)."""
    st = state256(F, L, bi, seed=1)
    e = _engine(st, F, L, bi)
    x = _x(B, T, F, seed=B + T)
    out = e.forward_host(x)
    _vs_f64(out, oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi), f"fp32 F={F} L={L} bi={bi}")
    # a window's rows are the same bits alone and inside the batch
    for b in (0, B - 1):
        assert np.array_equal(e.forward_host(x[b:b + 1]), out[b:b + 1]), b
    e.close()


# ---- half precision ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,L,bi", [(10, 2, True), (1, 1, False), (16, 4, True), (10, 3, False)])
def test_half_precision_vs_cpu_emulation(F, L, bi):
    st = state256(F, L, bi, seed=2)
    e = _engine(st, F, L, bi)
    e.set_precision(True)
    for B, T in ((7, 401), (40, 64)):
        x = _x(B, T, F, seed=3 * B + T)
        ref = oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi)
        out = e.forward_host(x)
        emu = _cpu_half_emulation(st, F, L, bi, x)
        dev, dev_emu = float(np.abs(out - ref).max()), float(np.abs(emu - ref).max())
        _WORST[f"half F={F} L={L} bi={bi} (CPU fp16 emulation {dev_emu:.2e})"] = dev
        assert np.isfinite(out).all()
        assert dev <= 2 * dev_emu, (dev, dev_emu)
        # argmax agreement with float64, on the columns whose top two float64 separates by more than twice the emulation's
        # deviation (a near-tie flips with any rounding: one such column of 2 560 does at F=10, L=3, uni)
        srt = np.sort(ref, -1)
        clear = (srt[..., -1] - srt[..., -2]) > 2 * dev_emu
        agree = float((out.argmax(-1) == ref.argmax(-1))[clear].mean())
        agree_emu = float((emu.argmax(-1) == ref.argmax(-1))[clear].mean())
        assert agree >= agree_emu, (agree, agree_emu)
        assert np.array_equal(e.forward_host(x), out), "two calls differ"
        assert np.array_equal(e.forward_host(x[1:2]), out[1:2]), "window alone vs in the batch"
    e.close()


@pytest.mark.parametrize("B,share", [(300, 1), (100, 4)], ids=["B300", "B100-share4"])
def test_half_precision_two_groups_per_cluster(B, share):
    """More groups of 16 windows than clusters: two interleaved groups per cluster (k_gru_wide<.., NGRP = 2, HP>).  300
    windows = 19 groups on at most 14 clusters per direction; gpu_share = 4 leaves 3 clusters per direction for 7 groups."""
    F, L, bi = 10, 2, True
    assert engine.pass_plan(B, 64, half=True, gru_size=H, gpu_share=share)["work_groups"] < 2 * 8 * -(-B // 16)
    st = state256(F, L, bi, seed=4)
    e = _engine(st, F, L, bi)
    e.set_option("gpu_share", share)
    e.set_precision(True)
    x = _x(B, 64, F, seed=B)
    ref = oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi)
    out = e.forward_host(x)
    emu = _cpu_half_emulation(st, F, L, bi, x)
    dev, dev_emu = float(np.abs(out - ref).max()), float(np.abs(emu - ref).max())
    _WORST[f"half NGRP=2 B={B} share={share} (CPU fp16 emulation {dev_emu:.2e})"] = dev
    assert np.isfinite(out).all() and dev <= 2 * dev_emu, (dev, dev_emu)
    assert np.array_equal(e.forward_host(x[B - 1:]), out[B - 1:]), "last window alone vs in the batch"
    e.close()


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_raw_counts_input(half):
    """Un-normalised counts (features.py's normalise=None): x far beyond fp16's reach once scaled.  Layer 0's projection is
    plain fp32, so the result is float64's, not NaN."""
    F, L, bi = 10, 2, True
    st = state256(F, L, bi, seed=5)
    e = _engine(st, F, L, bi)
    e.set_precision(half)
    x = synth.counts_windows(5, 300, seed=43) * np.float32(20000.0)
    assert x.max() > 4096
    out = e.forward_host(x)
    ref = oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi)
    _vs_f64(out, ref, f"raw counts {'half' if half else 'fp32'}", tol=2e-3 if half else TOL)
    x2 = _x(3, 200, F, seed=44)            # and normalised input afterwards
    _vs_f64(e.forward_host(x2), oracle.f64_gru_forward(x2, st, n_layers=L, bidirectional=bi), "after raw counts",
            tol=2e-3 if half else TOL)
    e.close()


# ---- the entries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_entries_agree_bitwise(half):
    F, L, bi = 10, 2, True
    st = state256(F, L, bi, seed=3)
    e = _engine(st, F, L, bi)
    e.set_precision(half)
    x = _x(9, 300, F, seed=5)
    out = e.forward_host(x)
    assert np.array_equal(_forward_dev(e, x), out), "device entry"
    assert np.array_equal(_forward_dev(e, x, "async"), out), "stream-ordered entry"
    assert np.array_equal(e.forward_host(x), out), "host entry after the stream-ordered one"
    # counts in, decoded out
    rng = np.random.default_rng(4)
    depth = rng.integers(0, 120, (4, 250)).astype(np.uint32)
    counts = rng.integers(0, np.maximum(depth, 1)[..., None] + 1, (4, 250, F)).astype(np.uint16)
    probs, cls, pmax = e.forward_counts_host(counts, depth, probs=True, decoded=True)
    xc = oracle.normalise_counts(counts, depth)
    assert np.array_equal(probs, e.forward_host(xc))
    assert np.array_equal(cls, probs.argmax(-1)) and np.array_equal(pmax, probs.max(-1))
    cls2, pmax2 = e.forward_decoded_host(xc)
    assert np.array_equal(cls2, cls) and np.array_equal(pmax2, pmax)
    # logits
    e.set_normalise(False)
    logits = e.forward_host(x)
    if not half:
        _vs_f64(logits, oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi, normalise=False), "fp32 logits", tol=1e-3)
    assert np.allclose(torch.softmax(torch.from_numpy(logits), -1).numpy(), out, atol=1e-6)
    assert np.array_equal(_forward_dev(e, x), logits)
    e.close()


def test_small_pass_budget_splits_the_batch():
    """max_rows_per_pass: the batch runs as several passes, same bits."""
    F, L, bi = 10, 2, True
    st = state256(F, L, bi, seed=6)
    e = _engine(st, F, L, bi)
    x = _x(20, 200, F, seed=6)
    out = e.forward_host(x)
    e.set_option("max_rows_per_pass", 7 * 200)
    assert np.array_equal(e.forward_host(x), out)
    e.set_option("wide_wait_ms", 1000)
    assert np.array_equal(e.forward_host(x), out)
    e.close()


def test_split_requested_runs_sequential(monkeypatch):
    """As tests/test_scan_split_gpu.py: MDK_SCAN_SPLIT cleared, the scan_split option set.  A GRU(256) call is not split."""
    monkeypatch.delenv("MDK_SCAN_SPLIT", raising=False)
    monkeypatch.delenv("MDK_SCAN_SPLIT_MARGIN", raising=False)
    monkeypatch.setenv("MDK_SCAN_SPLIT_ADAPT", "0")
    F, L, bi = 10, 2, True
    st = state256(F, L, bi, seed=7)
    e = _engine(st, F, L, bi)
    x = _x(4, 4096, F, seed=7)
    for mode in (1, 4):
        e.set_option("scan_split", mode)
        out = e.forward_host(x)
        info = e.split()
        assert info["status"] == "not used" and info["chunks"] == 1, info
        assert np.array_equal(_forward_dev(e, x, "async"), out)
        assert e.split()["status"] == "not used"
    e.set_option("scan_split", 0)
    assert np.array_equal(e.forward_host(x), out)
    _vs_f64(out, oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi), "fp32 split requested")
    e.close()


# ---- the model API ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,L,bi", [(10, 2, True), (7, 1, False)])
def test_model_api_strict(F, L, bi):
    st = state256(F, L, bi, seed=8)
    ref_model = ref_standins.GRUModel(num_features=F, gru_size=H, n_layers=L, bidirectional=bi)
    ref_model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    m = integration.convert(ref_model.to("cuda"), "cuda", strict=True)
    assert m is not ref_model and type(m).__module__ == "medaka_amd.models"
    x = _x(4, 700, F, seed=F + L)
    p = m.predict_on_batch(Batch(counts_matrix=torch.from_numpy(x)))
    assert p.dtype == torch.float32 and tuple(p.shape) == (4, 700, 5)
    _vs_f64(p.numpy(), oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi), f"model API F={F} L={L} bi={bi}")
    # the fed loop: Batch.collate stages each batch on the engine, predict_on_batch redeems it (staged / pipelined entries)
    m.engine()
    rng = np.random.default_rng(9)
    batches = [[types.SimpleNamespace(features=rng.random((300, F), dtype=np.float32)) for _ in range(5)] for _ in range(4)]
    host = [m.engine().forward_host(np.stack([s.features for s in b])) for b in batches]
    for b, want in zip(batches, host):
        got = m.predict_on_batch(Batch.collate(b)).numpy()
        assert np.array_equal(got, want)
    # half(): fp16 parameters, as the reference's; the CPU fp16 emulation of the same model is the yardstick
    m.half()
    st_half = {k: v.astype(np.float16).astype(np.float32) for k, v in st.items()}
    ph = m.predict_on_batch(Batch(counts_matrix=torch.from_numpy(x))).numpy()
    ref_h = oracle.f64_gru_forward(x, st_half, n_layers=L, bidirectional=bi)
    emu = _cpu_half_emulation(st_half, F, L, bi, x)
    assert float(np.abs(ph - ref_h).max()) <= 2 * float(np.abs(emu - ref_h).max())
