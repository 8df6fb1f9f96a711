"""Every GRUModel architecture the engine accepts (integration._gru_supported: 1..16 features, 1..4 layers, either direction),
against the float64 reference (`oracle.f64_gru_forward`, pinned in tests/test_oracle_arch_cpu.py).

Most of the GPU suite runs one model (10 features, 2 bidirectional layers).  Off that point the kernels take other branches:
  * F = 16: the bias row no longer fits the packed layer-0 block (K + 1 <= 16), layer 0 always runs k_gi_small, and a split
    scan gathers its virtual batch on every call; odd F: that gather copies scalars; F = 15: the bias sits in the block's
    last k-slot; F = 1: an almost empty block;
  * 3 or 4 bidirectional layers: layer 1's GEMM on the side stream into the second gi buffer, the activation ping-pong
    over more than two layers, the head behind the last layer's chunks;
  * one direction: the fused head on every launch and the head's D == 1 branches.
What is asserted: fp32 within 2e-5 of float64, half precision within 2e-3, argmax identity wherever the reference separates
its top two by twice the tolerance -- on every column for the (confident) trained weights; the regimes are pinned with
`engine.pass_plan`, and each regime's variants agree bit for bit where they run the same arithmetic."""
import math

import numpy as np
import pytest
import torch

from medaka_amd import engine, integration, synth
from medaka_amd.torch_ext import Batch
from oracle import oracle
import ref_standins
from test_parity_gpu import _check

pytestmark = pytest.mark.gpu
TOL, TOL_HALF = 2e-5, 2e-3
ARCHS = [(1, True), (1, False), (2, True), (2, False), (3, True), (3, False), (4, True), (4, False)]
ARCH_IDS = [f"L{L}{'bi' if bi else 'uni'}" for L, bi in ARCHS]

_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The largest |dp| against float64 per (F, layers, direction, precision), printed when the module ends."""
    yield
    print("\nworst max|dp| against float64:")
    for (F, L, bi, prec), err in sorted(_WORST.items()):
        print(f"  F={F:2d} L={L} {'bi ' if bi else 'uni'} {prec}: {err:.2e}")


def _vs_f64(out, ref, F, L, bi, half=False, what="", strict_argmax=False):
    err = float(np.abs(out - ref).max()) if out.size else 0.0
    key = (F, L, bi, "half" if half else "fp32")
    _WORST[key] = max(_WORST.get(key, 0.0), err)
    print(f"{what} F={F} L={L} {'bi' if bi else 'uni'} {'half' if half else 'fp32'}: max|dp| = {err:.2e}")
    _check(out, ref, tol=TOL_HALF if half else TOL, what=f"{what} F={F} L={L} bi={bi} half={half}",
           strict_argmax=strict_argmax)


def _engine(st, F, L, bi):
    return engine.GruEngine(st, num_features=F, n_layers=L, bidirectional=bi)


def _x(B, T, F, seed):
    return oracle.arch_input(synth.counts_windows(B, T, depth=40, seed=seed), F, seed=seed)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _forward_dev(e, x, entry="ptr", stream=None):
    """The device entries on torch buffers: "ptr" (mdk_gru_forward_dev) or "async" (mdk_gru_forward_dev_async)."""
    B, T, _ = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.empty((B, T, 5), dtype=torch.float32, device="cuda")
    call = e.forward_ptr if entry == "ptr" else e.forward_async_ptr
    call(xd.data_ptr(), B, T, yd.data_ptr(), stream=_stream() if stream is None else stream)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


@pytest.fixture
def product_default(monkeypatch):
    """As tests/test_scan_split_gpu.py: conftest pins the sequential scan; engines created under this fixture take the
    split scan the way a user's do, with a margin that does not move under bit-for-bit comparisons."""
    monkeypatch.delenv("MDK_SCAN_SPLIT", raising=False)
    monkeypatch.delenv("MDK_SCAN_SPLIT_MARGIN", raising=False)
    monkeypatch.setenv("MDK_SCAN_SPLIT_ADAPT", "0")


# ---- 1. the architecture grid ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,bi", ARCHS, ids=ARCH_IDS)
@pytest.mark.parametrize("F", [1, 7, 15, 16])
def test_architecture_grid(F, L, bi):
    """Small ragged shapes (B not a multiple of 8, odd T) in fp32 and half precision; the recurrence tile sizes compute
    the same bits."""
    st = oracle.arch_state(F, L, bi)
    e = _engine(st, F, L, bi)
    for B, T in ((1, 1), (3, 17), (9, 600)):
        x = _x(B, T, F, seed=100 * F + B + T)
        ref = oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi)
        for half in (False, True):
            e.set_precision(half)
            outs = []
            for tile in ((4, 8, 16) if half else (4, 8)):
                e.set_option("rec_windows_per_tile", tile)
                outs.append(e.forward_host(x))
            e.set_option("rec_windows_per_tile", 0)
            for o in outs[1:]:
                assert np.array_equal(o, outs[0]), (B, T, half)
            assert np.array_equal(e.forward_host(x), outs[0]), (B, T, half)
            _vs_f64(outs[0], ref, F, L, bi, half, what=f"grid {B}x{T}")
    e.close()


# ---- 2. the regimes of each architecture ------------------------------------------------------------------------------
REGIMES = [(7, 1, True), (16, 1, False), (16, 2, True), (7, 2, False), (7, 3, True), (16, 3, False), (16, 4, True),
           (7, 4, True), (7, 4, False)]


@pytest.mark.parametrize("F,L,bi", REGIMES, ids=[f"F{F}-L{L}{'bi' if bi else 'uni'}" for F, L, bi in REGIMES])
def test_regimes(F, L, bi):
    st = oracle.arch_state(F, L, bi)
    e = _engine(st, F, L, bi)
    e.enable_timing(True)
    fused_l0 = F + 1 <= 16
    # latency regime: 16 x 4096 on the sequential scan, layer 1's projection on the side stream (bidirectional, >= 2 layers);
    # the host entry streams x in (fused layer 0 only) and the probabilities out in slabs
    B, T = (16, 4096) if bi else (5, 2048)
    plan = engine.pass_plan(B, T, num_features=F, num_layers=L, bidirectional=bi, host_in=True, host_out=True)
    overlap = bi and L >= 2
    assert plan["fuse_layer0"] == fused_l0 and plan["overlap_gemm"] == overlap, plan
    assert plan["stream_in"] == (bi and fused_l0) and plan["stream_out"] == overlap, plan
    assert not plan["fuse_projection"], plan
    x = _x(B, T, F, seed=F * 7 + L)
    out = e.forward_host(x)
    e.set_option("overlap_gemm", 0)
    assert np.array_equal(e.forward_host(x), out), "overlap_gemm 0 vs 1"
    e.set_option("overlap_gemm", 1)
    e.set_option("stream_host", 0)
    assert np.array_equal(e.forward_host(x), out), "stream_host 0 vs 1"
    e.set_option("stream_host", 1)
    assert np.array_equal(_forward_dev(e, x), out), "host entry vs device entry"
    _vs_f64(out, oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi), F, L, bi, what=f"latency {B}x{T}")
    # throughput regime: 8-window tiles with the projections of layers >= 1 inside the recurrence kernel
    e.set_option("rec_windows_per_tile", 8)
    for B, T in ((13, 272), (6, 264)):
        x = _x(B, T, F, seed=F * 11 + L + T)
        ref = oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi)
        for half in (False, True):
            e.set_precision(half)
            e.set_option("fuse_head", 0)
            outs = {}
            for fp in (0, 2):
                e.set_option("fuse_proj", fp)
                outs[fp] = e.forward_host(x)
                assert e.timing()["fused_layers"] == (((1 << L) - 2) if fp else 0), (B, T, fp, e.timing())
            assert np.array_equal(outs[0], outs[2]), (B, T, half, float(np.abs(outs[0] - outs[2]).max()))
            e.set_option("fuse_head", 1)
            fused = e.forward_host(x)
            head = (256 | (512 if (T % 16 == 0 or not bi) else 0)) if L >= 2 else 0
            assert e.timing()["fused_layers"] == ((1 << L) - 2) | head, (B, T, e.timing())
            e.set_option("final_head", 0)
            assert np.array_equal(e.forward_host(x), fused), (B, T, half, "final_head 0 vs 1")
            assert e.timing()["fused_layers"] == ((1 << L) - 2) | (head & 256), (B, T, e.timing())
            e.set_option("final_head", 1)
            d = float(np.abs(fused - outs[0]).max())
            assert d <= (2e-3 if half else 1e-6), (B, T, half, d)
            assert np.array_equal(_forward_dev(e, x), fused), (B, T, half, "host entry vs device entry")
            _vs_f64(fused, ref, F, L, bi, half, what=f"throughput {B}x{T}")
    e.set_precision(False)
    e.close()


# ---- 3. padded features: the 10-feature trained model widened to 11..16 -----------------------------------------------
@pytest.mark.parametrize("pad", ["zero", "random"])
def test_padded_features_match_the_ten_feature_model(gold, pad):
    """Zero pad weights (with non-zero pad inputs), or non-zero pad weights with zero pad inputs, leave the trained model
    as it is.  At F = 16 layer 0 runs k_gi_small, which starts from the bias and adds x * w with fmaf in k order: a zero
    product adds an exact zero, so the result is the 10-feature model's unfused one bit for bit.  At F = 11..15 the fused
    block holds the bias in another k-slot: equal to 2e-6 (half precision: to its tolerance).  In fp32 every column's argmax
    is the float64 reference's."""
    st10 = gold["weights_trained"]
    e10 = engine.GruEngine(st10)
    e10u = engine.GruEngine(st10)
    e10u.set_option("fuse_l0", 0)
    for B, T in ((9, 600), (13, 2304), (16, 4096)):
        x10 = synth.counts_windows(B, T, seed=B + T)
        ref = oracle.f64_gru_forward(x10, st10)
        for half in (False, True):
            for e in (e10, e10u):
                e.set_precision(half)
            fused10, unfused10 = e10.forward_host(x10), e10u.forward_host(x10)
            _vs_f64(unfused10, ref, 10, 2, True, half, what=f"10 features unfused {B}x{T}", strict_argmax=not half)
            for F in range(11, 17):
                st = oracle.padded_state(st10, F, pad=pad, seed=F)
                x = oracle.arch_input(x10, F, pad=None if pad == "zero" else 0.0, seed=F)
                e = engine.GruEngine(st, num_features=F)
                e.set_precision(half)
                out = e.forward_host(x)
                e.close()
                if F == 16:
                    assert np.array_equal(out, unfused10), (pad, B, T, half, float(np.abs(out - unfused10).max()))
                else:
                    d = float(np.abs(out - fused10).max())
                    assert d <= (TOL_HALF if half else 2e-6), (pad, F, B, T, half, d)
                _vs_f64(out, ref, F, 2, True, half, what=f"padded ({pad}) {B}x{T}", strict_argmax=not half)
    e10.close()
    e10u.close()


# ---- 4. the split scan off the default width ---------------------------------------------------------------------------
@pytest.mark.parametrize("F", [11, 15, 16])
def test_split_scan_off_the_default_width(gold, product_default, F):
    """Trained weights widened to F (odd F: the virtual-batch gather copies scalars; F = 16: layer 0 is never fused, so the
    gather runs on every call).  Certified calls agree with the sequential scan to 2e-6 and with float64 to 2e-5; the host,
    device and stream-ordered entries deliver the same bits; input beyond fp16 range takes the exact projection."""
    st = oracle.padded_state(gold["weights_trained"], F, pad="random", seed=F)
    e = engine.GruEngine(st, num_features=F)
    for B, T in ((16, 4096), (200, 2256)):
        x = _x(B, T, F, seed=F + T)
        out = e.forward_host(x)
        info = e.split()
        assert info["status"] == "certified" and info["chunks"] >= 2, (B, T, info)
        e.set_option("scan_split", 0)
        seq = e.forward_host(x)
        assert e.split()["status"] == "not used"
        e.set_option("scan_split", 1)
        assert float(np.abs(out - seq).max()) <= 2e-6, (B, T, float(np.abs(out - seq).max()))
        sub = slice(None) if B <= 16 else slice(0, B, 10)         # (windows are independent: float64 on every 10th one)
        _vs_f64(out[sub], oracle.f64_gru_forward(x[sub], st), F, 2, True, what=f"split {B}x{T}")
        assert np.array_equal(_forward_dev(e, x), out), (B, T, "device entry")
        assert e.split()["status"] == "certified"
        assert np.array_equal(_forward_dev(e, x, "async"), out), (B, T, "stream-ordered entry")
        assert e.split()["status"] == "certified"
    if F % 2:
        # raw counts: beyond the fused projection's fp16 range, layer 0 falls back on the device to the exact projection over
        # the gathered virtual batch
        x = _x(16, 4096, F, seed=5) * np.float32(3000.0)
        out = e.forward_host(x)
        info = e.split()
        assert info["chunks"] >= 2 and info["status"] in ("certified", "rejected"), info
        _vs_f64(out, oracle.f64_gru_forward(x, st), F, 2, True, what=f"split, raw counts ({info['status']})")
        x = _x(16, 4096, F, seed=6)
        out = e.forward_host(x)
        _vs_f64(out, oracle.f64_gru_forward(x, st), F, 2, True, what="split, after raw counts")
        if info["status"] == "certified":         # (a rejected call leaves the model on the sequential scan: auto mode)
            assert e.split()["status"] == "certified", e.split()
    e.close()


# ---- 5. counts in, decoded out -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,L,bi", [(7, 1, False), (7, 3, True), (16, 4, True), (16, 2, False)])
def test_counts_and_decoded_entries(F, L, bi):
    rng = np.random.default_rng(F * 10 + L)
    B, T = 5, 333
    depth = rng.integers(0, 120, (B, T)).astype(np.uint32)
    counts = rng.integers(0, np.maximum(depth, 1)[..., None] + 1, (B, T, F)).astype(np.uint16)
    st = oracle.arch_state(F, L, bi)
    e = _engine(st, F, L, bi)
    probs, cls, pmax = e.forward_counts_host(counts, depth, probs=True, decoded=True)
    x = oracle.normalise_counts(counts, depth)
    assert np.array_equal(probs, e.forward_host(x))
    _vs_f64(probs, oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi), F, L, bi, what="counts in")
    assert np.array_equal(cls, probs.argmax(-1)) and np.array_equal(pmax, probs.max(-1))
    cls2, pmax2 = e.forward_decoded_host(x)
    assert np.array_equal(cls2, cls) and np.array_equal(pmax2, pmax)
    assert np.array_equal(e.forward_counts_host(counts, depth), probs)
    e.close()


# ---- 6. the stream-ordered entry outside the split ---------------------------------------------------------------------
@pytest.mark.parametrize("L,bi", [(1, True), (3, True), (4, True), (2, False), (4, False)],
                         ids=["L1bi", "L3bi", "L4bi", "L2uni", "L4uni"])
def test_stream_ordered_entry_outside_the_split(product_default, L, bi):
    F = 16
    st = oracle.arch_state(F, L, bi)
    e = _engine(st, F, L, bi)
    shapes = ((9, 600), (3, 1000)) + (() if bi else ((16, 4096),))
    xs = [_x(B, T, F, seed=L * 100 + B) for B, T in shapes]
    sync = []
    for x in xs:
        sync.append(_forward_dev(e, x))
        assert e.split()["status"] == "not used", x.shape
        assert np.array_equal(_forward_dev(e, x, "async"), sync[-1]), x.shape
        assert e.split()["status"] == "not used", x.shape
    _vs_f64(sync[0], oracle.f64_gru_forward(xs[0], st, n_layers=L, bidirectional=bi), F, L, bi, what="stream-ordered")
    # several calls in flight on two streams
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    xd = [torch.from_numpy(x).cuda() for x in xs]
    torch.cuda.synchronize()
    ys = []
    for rep in range(3):
        for i, x in enumerate(xd):
            s = streams[(rep + i) % 2]
            y = torch.empty(x.shape[:2] + (5,), dtype=torch.float32, device="cuda")
            e.forward_async_ptr(x.data_ptr(), x.shape[0], x.shape[1], y.data_ptr(), stream=s.cuda_stream)
            ys.append((i, y))
    torch.cuda.synchronize()
    for i, y in ys:
        assert np.array_equal(y.cpu().numpy(), sync[i]), (i, xs[i].shape)
    assert e.split()["status"] == "not used"
    e.close()


# ---- 7. fused layer-0 packing refused at load time ---------------------------------------------------------------------
def _x_scale(st, bidirectional=True):
    """The layer-0 packing scale mdk_gru_create picks (gru_model.hpp): W_hh's power-of-two scale sw puts max |W_hh| * sw in
    [2^13, 2^14) (shift clamped to [-10, 14]), S = 1024 sw, and sx doubles from 16 until sx >= S * max(|W_ih|, |folded
    bias|) / 2^15.  Above 8192 the fused projection is not packed."""
    sx = 16.0
    for sfx in ([""] + (["_reverse"] if bidirectional else [])):
        _, ex = math.frexp(float(np.abs(st[f"gru.weight_hh_l0{sfx}"]).max()))
        S = 1024.0 * 2.0 ** max(-10, min(14, 14 - ex))
        bias = st[f"gru.bias_ih_l0{sfx}"] + np.concatenate([st[f"gru.bias_hh_l0{sfx}"][:256], np.zeros(128, np.float32)])
        mx = max(float(np.abs(st[f"gru.weight_ih_l0{sfx}"]).max()), float(np.abs(bias).max()))
        while sx < S * mx / 32768.0:
            sx *= 2.0
    return sx


def test_fused_layer0_refused_beyond_its_packing_scale():
    base = oracle.arch_state(10, 2, True)
    assert _x_scale(base) <= 8192.0
    # the smallest power-of-two gain on W_ih that takes sx past 8192: at half of it the fused path is still packed
    g = 2.0 ** math.ceil(math.log2(8192.0 / _x_scale(base)))
    while True:
        st = dict(base)
        for sfx in ("", "_reverse"):
            st[f"gru.weight_ih_l0{sfx}"] = base[f"gru.weight_ih_l0{sfx}"] * np.float32(g)
        if _x_scale(st) > 8192.0:
            break
        g *= 2.0
    below = dict(st)
    for sfx in ("", "_reverse"):
        below[f"gru.weight_ih_l0{sfx}"] = base[f"gru.weight_ih_l0{sfx}"] * np.float32(g / 2)
    assert _x_scale(below) <= 8192.0 < _x_scale(st), (g, _x_scale(below), _x_scale(st))
    x = synth.counts_windows(9, 600, seed=71)
    for state, refused in ((st, True), (below, False)):
        ref = oracle.f64_gru_forward(x, state)
        e, eu = engine.GruEngine(state), engine.GruEngine(state)
        eu.set_option("fuse_l0", 0)
        a, b = e.forward_host(x), eu.forward_host(x)
        e.close()
        eu.close()
        # refused: the default engine runs the unfused projection -- the same bits; packed: the fused MFMA projection
        # rounds differently somewhere in 27 000 probabilities
        assert np.array_equal(a, b) == refused, (g, refused, float(np.abs(a - b).max()))
        _vs_f64(a, ref, 10, 2, True, what=f"W_ih x {g if refused else g / 2:g}")


# ---- 8. through the model API ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,L,bi", [(16, 4, True), (7, 1, False)])
def test_model_api_off_the_default_architecture(F, L, bi):
    st = oracle.arch_state(F, L, bi)
    ref_model = ref_standins.GRUModel(num_features=F, n_layers=L, bidirectional=bi)
    ref_model.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=True)
    m = integration.convert(ref_model, "cuda", strict=True)
    assert m is not ref_model and type(m).__module__ == "medaka_amd.models"
    x = _x(4, 700, F, seed=F + L)
    ref = oracle.f64_gru_forward(x, st, n_layers=L, bidirectional=bi)
    p = m.predict_on_batch(Batch(counts_matrix=torch.from_numpy(x)))
    assert p.dtype == torch.float32 and tuple(p.shape) == (4, 700, 5)
    _vs_f64(p.numpy(), ref, F, L, bi, what="model API")
    # half(): the parameters themselves become fp16 (as the reference's do): the yardstick is float64 on those
    m.half()
    st_half = {k: v.astype(np.float16).astype(np.float32) for k, v in st.items()}
    _vs_f64(m.predict_on_batch(Batch(counts_matrix=torch.from_numpy(x))).numpy(),
            oracle.f64_gru_forward(x, st_half, n_layers=L, bidirectional=bi), F, L, bi, half=True, what="model API")
