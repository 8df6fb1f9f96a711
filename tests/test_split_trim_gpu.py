"""The last layer's scan range of a split call (option "scan_split_trim", gru_split.hpp `plan_scan_ranges`, rec_fused.hpp `rng`).

A chunk is run over its core plus one margin on either side, but the LAST layer scans only the columns somebody reads:
  * level 1 drops the trailing outer half-margin -- nothing reads it, and every state that is still computed has the same
    inputs: probabilities and `split()` records must be BIT-IDENTICAL to level 0 (the whole virtual window), through the device
    entry, the host entry (result streamed out under the scan), the stream-ordered entry, in both precisions;
  * level 2 also starts the last layer half a margin later: results differ at the rounding-noise level, as results at two
    margins do -- checked against the float64 C oracle at the parity tolerance, against the engine's own sequential scan within
    the audit tolerance (1e-5; 4e-4 in half precision) with every argmax, host and device entries bit-identical to each other;
  * a certificate that is rejected at level 2 is retried and falls back exactly as at level 0.
Every shape here runs the last layer in the form the trim applies to (the scan's second half writes the probabilities itself,
`fused_layers` bit 9): that is asserted, so that none of this passes by comparing the untrimmed path with itself."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLD
from medaka_amd import engine, synth
from oracle import oracle
from test_parity_gpu import _check

pytestmark = pytest.mark.gpu

# 200 x 10 000 (BASELINE configs[1]: 5 chunks, every recurrence tile inside one chunk), 100 x 10 000 (the reference CLI's default
# batch: 10 chunks, tiles that mix two chunks), a batch that is no multiple of 8 (68: 15 chunks), and a forced chunk count of 16
SHAPES = [(200, 10000, 1), (100, 10000, 1), (68, 10000, 1), (60, 10000, 16)]
IDS = ["200x10000", "100x10000", "68x10000", "60x10000-forced16"]


@pytest.fixture(autouse=True)
def product_default(monkeypatch):
    """conftest turns the split off for the older tests; here it is on, at a margin that does not move under a bit-for-bit
    comparison, and the trim level is the one each test sets."""
    monkeypatch.delenv("MDK_SCAN_SPLIT", raising=False)
    monkeypatch.delenv("MDK_SCAN_SPLIT_MARGIN", raising=False)
    monkeypatch.delenv("MDK_SCAN_SPLIT_TRIM", raising=False)
    monkeypatch.setenv("MDK_SCAN_SPLIT_ADAPT", "0")


def _windows(B, T, seed):
    return np.concatenate([synth.counts_windows(min(8, B - b), T, depth=50, seed=seed + b) for b in range(0, B, 8)])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _engine(st, trim, scan_split=1, half=False):
    e = engine.GruEngine(st)
    e.set_precision(half)
    e.set_option("scan_split_trim", trim)
    if scan_split != 1:
        e.set_option("scan_split", scan_split)
    e.enable_timing(True)
    return e


def _all_entries(e, x, xd):
    """The same call through the device entry, the host entry and the stream-ordered entry: [(probabilities, split record)]."""
    B, T, _ = x.shape
    res = []
    yd = torch.empty(B, T, 5, device="cuda")
    e.forward_ptr(xd.data_ptr(), B, T, yd.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    assert e.timing()["fused_layers"] & 512, e.timing()             # the form the trim applies to
    res.append((yd.cpu().numpy(), e.split()))
    host = e.forward_host(x)
    assert e.timing()["host_streamed"] & 2, e.timing()              # ... and its result left in column chunks under the scan
    res.append((host, e.split()))
    yd.zero_()
    e.forward_async_ptr(xd.data_ptr(), B, T, yd.data_ptr(), stream=_stream())
    info = e.split()                                                # (waits for the call)
    torch.cuda.synchronize()
    res.append((yd.cpu().numpy(), info))
    return res


@pytest.mark.parametrize("B,T,scan_split", SHAPES, ids=IDS)
def test_trailing_trim_is_bit_identical(gold, B, T, scan_split):
    """Level 1 against level 0: two fresh engines, the same calls in the same order (so that audits and probes fall on the
    same calls), fp32 parity then half precision."""
    x = _windows(B, T, 500)
    xd = torch.from_numpy(x).cuda()
    runs = {}
    for trim in (0, 1):
        e = _engine(gold["weights_trained"], trim, scan_split)
        runs[trim] = _all_entries(e, x, xd)
        e.set_precision(True)
        runs[trim] += _all_entries(e, x, xd)
        e.close()
    names = [f"{p} {n}" for p in ("fp32", "half") for n in ("device entry", "host entry", "stream-ordered entry")]
    for name, (p0, i0), (p1, i1) in zip(names, runs[0], runs[1]):
        assert i0["status"] == "certified" and i0["chunks"] >= 5, (name, i0)
        assert i1 == i0, (name, i0, i1)
        assert np.array_equal(p1, p0), (name, float(np.abs(p1 - p0).max()))
    for k in (1, 2, 4, 5):                                          # ... and the entries agree with each other, as ever
        assert np.array_equal(runs[1][k][0], runs[1][k - k % 3][0]), names[k]


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("B,T,scan_split", SHAPES, ids=IDS)
def test_leading_trim_vs_oracle_and_sequential(gold, B, T, scan_split, half):
    """Level 2, the round-1 trained set (whose certificate holds): a sample of windows (first and last tile, tiles that
    mix chunks) against the float64 C oracle at the parity tolerance with every argmax (fp32 parity), all columns against the
    engine's own sequential scan within the audit tolerance with every argmax, host entry = device entry bit for bit."""
    st = gold["weights_trained"]
    x = _windows(B, T, 700)
    xd = torch.from_numpy(x).cuda()
    e = _engine(st, 2, scan_split, half)
    (dev, info), (host, info_h), (asy, info_a) = _all_entries(e, x, xd)
    assert info["status"] == "certified" and info["chunks"] >= 2, info
    assert info_h["status"] == "certified" and info_a["status"] == "certified", (info_h, info_a)
    assert np.array_equal(host, dev) and np.array_equal(asy, dev)
    e.set_option("scan_split", 0)
    seq = e.forward_host(x)
    assert e.split()["status"] == "not used"
    e.close()
    d = float(np.abs(dev - seq).max())
    print(f"{B} x {T} half={half} trim 2: {info['chunks']} chunks, largest junction difference {info['max_delta']:.2e}, "
          f"max|dp| vs the sequential scan {d:.2e}")
    assert d <= (4e-4 if half else 1e-5), d                         # scan_split.hpp kAuditTolHalf / kAuditTol
    assert np.array_equal(dev.argmax(-1), seq.argmax(-1))
    if not half:
        idx = sorted({0, 7, 8, B // 8 * 8 - 1, B // 2, B // 2 + 1, B - 9, B - 8, B - 1})
        ref = oracle.c_gru_forward(np.ascontiguousarray(x[idx]), st)
        _check(dev[idx], ref, what=f"trim 2, {B} x {T}, windows {idx} vs the C oracle", strict_argmax=True)


def test_rejected_certificate_with_the_leading_trim(gold):
    """A model that latches state never certifies: at level 2 the call climbs the same ladder, is answered with the sequential
    scan's bits and leaves the model on the sequential scan, exactly as at level 0."""
    zoo = np.load(os.path.join(GOLD, "weights_zoo.npz"))
    st = {k[len("latch/"):]: zoo[k] for k in zoo.files if k.startswith("latch/")}
    assert st, zoo.files[:5]
    B, T = 200, 10000
    x = _windows(B, T, 900)
    got = {}
    for trim in (0, 2):
        e = _engine(st, trim)
        out = e.forward_host(x)
        info = e.split()
        e.forward_host(x)
        after = e.split()
        e.set_option("scan_split", 0)
        seq = e.forward_host(x)
        e.close()
        assert info["status"] == "rejected" and info["fallbacks"] == 5 and info["margin"] == 512, (trim, info)
        assert after["status"] == "disabled" and after["fallbacks"] == 5, (trim, after)
        assert np.array_equal(out, seq), trim
        got[trim] = (out, {k: info[k] for k in ("status", "chunks", "margin", "columns", "fallbacks", "audited", "audits")})
    assert got[2][1] == got[0][1], got
    assert np.array_equal(got[2][0], got[0][0])
