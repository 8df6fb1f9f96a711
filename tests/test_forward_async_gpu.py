"""The stream-ordered device forward (`mdk_gru_forward_dev_async`): the split scan's certificate,
the sequential repair of a rejected call, the half-precision probe and the audit are decided on the device, and the call
returns as soon as it is enqueued.

What is asserted:
  * the host does not wait: behind a >= 150 ms GPU sleep the call returns within 20 ms and its work is still pending --
    where the synchronous device entry waits for the whole sleep;
  * certified calls deliver the synchronous entry's bits at the same margin; rejected calls deliver the sequential scan's
    bits, and the learner takes its step once the call is retired;
  * input beyond fp16 range, the half-precision probe, the audit, two streams with a small ring, the host entries around
    it and the model API all stay correct."""
import ctypes
import os
import time

import numpy as np
import pytest
import torch

from conftest import GOLD, weight_set
from medaka_amd import engine, lib, models, synth
from test_parity_gpu import _check

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def product_default(monkeypatch):
    """As tests/test_scan_split_gpu.py: engines are created the way a user's are, with a margin that does not move under
    bit-for-bit comparisons."""
    monkeypatch.delenv("MDK_SCAN_SPLIT", raising=False)
    monkeypatch.delenv("MDK_SCAN_SPLIT_MARGIN", raising=False)
    monkeypatch.setenv("MDK_SCAN_SPLIT_ADAPT", "0")


_SLEEP = {}


def _sleep_cycles():
    """torch.cuda._sleep cycles that take at least 150 ms on this GPU (measured once with CUDA events)."""
    if "n" not in _SLEEP:
        n = 20_000_000
        for _ in range(6):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(n)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 150.0:
                break
            n = int(n * max(2.0, 1.3 * 150.0 / max(ms, 1e-3)))
        assert ms >= 150.0, ms
        _SLEEP["n"] = n
    return _SLEEP["n"]


def _host_time_behind_sleep(call):
    """Run `call` behind a >= 150 ms GPU sleep on the current stream: (host seconds of the call, whether an event recorded
    right after it was still pending when the call returned)."""
    torch.cuda.synchronize()
    torch.cuda._sleep(_sleep_cycles())
    t0 = time.perf_counter()
    call()
    dt = time.perf_counter() - t0
    ev = torch.cuda.Event()
    ev.record()
    pending = not ev.query()
    torch.cuda.synchronize()
    return dt, pending


def _assert_no_wait(call):
    dt, pending = _host_time_behind_sleep(call)
    assert dt < 0.020 and pending, f"the call took {dt * 1e3:.1f} ms of host time (work still pending: {pending})"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _async(e, x_d, out_d, stream=None):
    B, T, _ = x_d.shape
    e.forward_async_ptr(x_d.data_ptr(), B, T, out_d.data_ptr(), stream=_stream() if stream is None else stream)


def _sync(e, x_d):
    B, T, _ = x_d.shape
    out = torch.empty((B, T, 5), dtype=torch.float32, device=x_d.device)
    e.forward_ptr(x_d.data_ptr(), B, T, out.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _sync_learner_after_one_rejection(g0):
    """The margin the synchronous entry's learner (the same state machine, run device-free as mdk_margin_sim) tries after
    ONE rejection at g0: a model that certifies from g0 + 8 on answers its first call at exactly that margin."""
    margins, forwards = (ctypes.c_int * 1)(), (ctypes.c_int * 1)()
    lib.check(lib.load().mdk_margin_sim(g0, 0, g0 + 8, 1, margins, forwards), "mdk_margin_sim")
    assert forwards[0] == 2, (g0, forwards[0])
    return margins[0]


def _calls_until_split(call, e, limit=200):
    """Calls (each followed by split()) until one runs as a split scan again: the back-off's length as the caller sees it."""
    for n in range(1, limit + 1):
        call()
        info = e.split()
        if info["status"] != "disabled":
            return n, info
    return None, info


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_the_host_does_not_wait(gold, half):
    """A certifying 200 x 10 000 batch behind a 150 ms GPU sleep: the async call returns within 20 ms with its work
    pending, and delivers the synchronous entry's bits at the same margin; the synchronous entry waits out the sleep."""
    B, T = 200, 10000
    x = _dev(synth.counts_windows(B, T, seed=11))
    ea = engine.GruEngine(weight_set(gold, "trained"))
    es = engine.GruEngine(weight_set(gold, "trained"))
    ea.set_precision(half)
    es.set_precision(half)
    out = torch.empty((B, T, 5), dtype=torch.float32, device="cuda")
    _async(ea, x, out)                             # warm-up: workspace, probe, first audit
    torch.cuda.synchronize()
    assert ea.split()["status"] == "certified", ea.split()
    out.zero_()
    _assert_no_wait(lambda: _async(ea, x, out))
    info = ea.split()
    want = _sync(es, x)
    ref = es.split()
    assert info["status"] == "certified" and ref["status"] == "certified", (info, ref)
    assert info["margin"] == ref["margin"] and info["chunks"] == ref["chunks"], (info, ref)
    assert np.array_equal(out.cpu().numpy(), want)
    # the yardstick itself: the synchronous device entry does wait for the sleep in front of it
    o2 = torch.empty_like(out)
    dt, _ = _host_time_behind_sleep(lambda: es.forward_ptr(x.data_ptr(), B, T, o2.data_ptr(), stream=_stream()))
    assert dt >= 0.1, dt
    ea.close()
    es.close()


@pytest.mark.parametrize("name", ["x5", "saturated"])
def test_a_rejected_call_is_repaired_on_the_device(gold, name):
    """Weights whose memory outlasts every margin: the async call's own result is the sequential scan's, bit for bit; once
    retired, the rejection moves the learner one step, and the next call runs at the next margin of the ladder."""
    from oracle.make_golden_adversarial import adversarial_state
    st = adversarial_state(name, gold["weights_init"], gold["weights_trained"])
    B, T = 16, 4096
    x = _dev(synth.counts_windows(B, T, seed=5))
    ea = engine.GruEngine(st)
    eq = engine.GruEngine(st)
    eq.set_option("scan_split", 0)
    want = _sync(eq, x)
    out = torch.full((B, T, 5), -1.0, dtype=torch.float32, device="cuda")
    _async(ea, x, out)
    info = ea.split()
    assert info["status"] == "rejected" and info["fallbacks"] >= 1 and info["chunks"] >= 2, info
    assert np.array_equal(out.cpu().numpy(), want)
    g0 = info["margin"]
    out.fill_(-1.0)
    _async(ea, x, out)
    nxt = ea.split()
    assert np.array_equal(out.cpu().numpy(), want)
    # the synchronous entry's learner after one rejection at g0 (a rejection there goes on up)
    assert nxt["margin"] == _sync_learner_after_one_rejection(g0), (info, nxt)
    assert nxt["status"] == "rejected" and nxt["fallbacks"] == info["fallbacks"] + 1, nxt
    ea.close()
    eq.close()


def test_rejections_in_flight_start_one_back_off(gold):
    """Eight calls in flight at the largest margin, all rejected by weights that never forget: their retirement starts ONE
    back-off, and the split is tried again after as many calls as after the synchronous entry's single rejection -- not
    after a back-off doubled by every call that was in flight."""
    from oracle.make_golden_adversarial import adversarial_state
    st = adversarial_state("saturated", gold["weights_init"], gold["weights_trained"])
    B, T = 16, 4096
    x = _dev(synth.counts_windows(B, T, seed=6))
    out = torch.empty((B, T, 5), dtype=torch.float32, device="cuda")
    es = engine.GruEngine(st)
    es.set_option("scan_split_margin", 512)      # the top of the ladder: one rejection gives the model up
    ea = engine.GruEngine(st)
    ea.set_option("scan_split_margin", 512)
    es.forward_ptr(x.data_ptr(), B, T, out.data_ptr(), stream=_stream())
    first = es.split()
    assert first["status"] == "rejected" and first["margin"] == 512 and first["chunks"] >= 2, first
    n_sync, again_sync = _calls_until_split(lambda: es.forward_ptr(x.data_ptr(), B, T, out.data_ptr(), stream=_stream()), es)
    _async(ea, x, out)                           # warm-up of the workspace at this shape: rejected, starts the back-off
    warm = ea.split()
    ea.set_option("scan_split_margin", 512)      # (re-arms the model: back-off and learner as new)
    torch.cuda._sleep(_sleep_cycles())           # nothing of the burst can finish -- and be retired -- while it is enqueued
    for _ in range(8):                           # the default ring holds all eight
        _async(ea, x, out)
    burst = ea.split()
    assert burst["status"] == "rejected" and burst["margin"] == 512 and burst["fallbacks"] == warm["fallbacks"] + 8, burst
    n_async, again_async = _calls_until_split(lambda: _async(ea, x, out), ea)
    assert n_sync == 64 and n_async == n_sync, (n_sync, n_async)
    assert again_async["status"] == again_sync["status"] == "rejected" and again_async["margin"] == 512, (again_sync, again_async)
    ea.close()
    es.close()


def test_input_beyond_fp16_range_is_decided_on_the_device(gold):
    """The adversarial range goldens through the async entry: within the tolerance the synchronous split is held to against
    the unmodified reference, and without a host wait."""
    from oracle.make_golden_adversarial import adversarial_input, adversarial_state
    adv = np.load(os.path.join(GOLD, "gru_adversarial.npz"))
    for name in ("bigx", "range16"):
        e = engine.GruEngine(adversarial_state(name, gold["weights_init"], gold["weights_trained"]))
        x = _dev(adversarial_input(name))
        out = torch.empty((x.shape[0], x.shape[1], 5), dtype=torch.float32, device="cuda")
        _async(e, x, out)                         # warm-up
        torch.cuda.synchronize()
        out.zero_()
        _assert_no_wait(lambda: _async(e, x, out))
        info = e.split()
        assert info["status"] in ("certified", "rejected"), info
        _check(out.cpu().numpy(), adv[name], tol=1e-4, what=f"{name} async {info}", strict_argmax=True)
        e.close()


def test_half_precision_probe_in_stream_order(gold):
    """Six async calls of a fresh half-precision engine back to back: one probe serves them all (<= 2), every call was
    delivered at a margin whose probe certified, and every result is within 2e-4 of the fp32 result, argmax identical."""
    B, T = 200, 4000
    xs = [_dev(synth.counts_windows(B, T, seed=100 + i)) for i in range(6)]
    e = engine.GruEngine(weight_set(gold, "trained"))
    e.set_precision(True)
    ef = engine.GruEngine(weight_set(gold, "trained"))
    outs = [torch.empty((B, T, 5), dtype=torch.float32, device="cuda") for _ in xs]
    for x, o in zip(xs, outs):
        _async(e, x, o)
    torch.cuda.synchronize()
    info = e.split()
    assert 1 <= info["probes"] <= 2, info
    assert info["status"] == "certified" and info["probe_max_delta"] <= 3.814697265625e-06, info
    for x, o in zip(xs, outs):
        want = _sync(ef, x)
        got = o.cpu().numpy()
        assert np.abs(got - want).max() <= 2e-4
        assert np.array_equal(got.argmax(-1), want.argmax(-1))
    e.close()
    ef.close()


def test_audit_in_stream_order(gold):
    """The first async call of a fresh engine is audited (<= 4e-6 in fp32); with "scan_split_audit" = 2 every call is, and
    the results keep the bits of an engine that audits nothing."""
    B, T = 200, 4000
    xs = [_dev(synth.counts_windows(B, T, seed=200 + i)) for i in range(3)]
    e = engine.GruEngine(weight_set(gold, "trained"))
    out = torch.empty((B, T, 5), dtype=torch.float32, device="cuda")
    _async(e, xs[0], out)
    info = e.split()
    assert info["status"] == "certified" and info["audited"] and info["audit_max_dp"] <= 4e-6 and info["audits"] == 1, info
    e.close()
    ea = engine.GruEngine(weight_set(gold, "trained"))
    ea.set_option("scan_split_audit", 2)
    en = engine.GruEngine(weight_set(gold, "trained"))
    en.set_option("scan_split_audit", 0)
    for i, x in enumerate(xs):
        oa = torch.empty((B, T, 5), dtype=torch.float32, device="cuda")
        on = torch.empty_like(oa)
        _async(ea, x, oa)
        _async(en, x, on)
        ia, inn = ea.split(), en.split()
        assert ia["audited"] and ia["audits"] == i + 1 and ia["audit_failures"] == 0, ia
        assert not inn["audited"] and inn["audits"] == 0, inn
        assert np.array_equal(oa.cpu().numpy(), on.cpu().numpy())
    ea.close()
    en.close()


def test_two_streams_and_a_small_ring(gold):
    """Twelve calls alternating between two streams, three inputs, "async_depth" = 4 and an audit behind every call: each
    output holds its own input's synchronous result -- no later call's repair or audit writes over it."""
    B, T = 200, 4000
    xs = [_dev(synth.counts_windows(B, T, seed=300 + i)) for i in range(3)]
    e = engine.GruEngine(weight_set(gold, "trained"))
    e.set_option("async_depth", 4)
    e.set_option("scan_split_audit", 2)
    es = engine.GruEngine(weight_set(gold, "trained"))
    want = [_sync(es, x) for x in xs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for i in range(12):
        s = streams[i % 2]
        with torch.cuda.stream(s):
            o = torch.full((B, T, 5), -1.0, dtype=torch.float32, device="cuda")
            _async(e, xs[i % 3], o, stream=s.cuda_stream)
        outs.append(o)
    torch.cuda.synchronize()
    info = e.split()
    assert info["status"] == "certified" and info["audits"] == 12 and info["audit_failures"] == 0, info
    for i, o in enumerate(outs):
        assert np.array_equal(o.cpu().numpy(), want[i % 3]), i
    e.close()
    es.close()


def test_two_streams_and_a_small_ring_with_rejected_calls(gold):
    """As above with weights the certificate rejects: every call's repair runs, the learner climbs and gives up while
    calls are in flight, and each output still holds its own input's sequential scan."""
    from oracle.make_golden_adversarial import adversarial_state
    st = adversarial_state("x5", gold["weights_init"], gold["weights_trained"])
    B, T = 16, 4096
    xs = [_dev(synth.counts_windows(B, T, seed=500 + i)) for i in range(3)]
    e = engine.GruEngine(st)
    e.set_option("async_depth", 4)
    eq = engine.GruEngine(st)
    eq.set_option("scan_split", 0)
    want = [_sync(eq, x) for x in xs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    outs = []
    for i in range(12):
        s = streams[i % 2]
        with torch.cuda.stream(s):
            o = torch.full((B, T, 5), -1.0, dtype=torch.float32, device="cuda")
            _async(e, xs[i % 3], o, stream=s.cuda_stream)
        outs.append(o)
    torch.cuda.synchronize()
    info = e.split()
    assert info["fallbacks"] >= 4, info
    for i, o in enumerate(outs):
        assert np.array_equal(o.cpu().numpy(), want[i % 3]), i
    e.close()
    eq.close()


def test_mixing_with_the_host_entries(gold):
    """A pipelined staged sequence with a batch started ahead, then an async call (which drops that batch first), then the
    host entry: every result is right."""
    B, T = 100, 4000
    xs = [synth.counts_windows(B, T, seed=400 + i) for i in range(3)]
    e = engine.GruEngine(weight_set(gold, "trained"))
    es = engine.GruEngine(weight_set(gold, "trained"))
    want = [es.forward_host(x) for x in xs]
    pins = [engine.PinnedArray((B, T, 10)) for _ in range(2)]
    outs = [engine.PinnedArray((B, T, 5)) for _ in range(2)]
    for p, x in zip(pins, xs):
        p.array[...] = x
    toks = [e.stage_input(p.array.ctypes.data, B, T) for p in pins]
    assert all(toks)
    assert e.forward_staged(toks[0], B, T, outs[0].array.ctypes.data, next_out_ptr=outs[1].array.ctypes.data)
    assert np.array_equal(outs[0].array, want[0])
    # the second batch may now be running ahead; the async call drops it before it enqueues anything
    x_d = _dev(xs[2])
    o = torch.empty((B, T, 5), dtype=torch.float32, device="cuda")
    _async(e, x_d, o)
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), want[2])
    assert not e.forward_staged(toks[1], B, T, outs[1].array.ctypes.data)     # its token was spent by the drop
    assert np.array_equal(e.forward_host(xs[1]), want[1])
    _async(e, x_d, o)                            # and once more, with the host entry right behind it (no synchronize between)
    assert np.array_equal(e.forward_host(xs[0]), want[0])
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), want[2])
    e.close()
    es.close()


def test_model_api_stream_ordered(gold):
    """GRUModel with `stream_ordered` = True: model(x) does not wait on the host and equals the default forward bit for bit."""
    state = {k: torch.from_numpy(v) for k, v in gold["weights_trained"].items()}
    m_async = models.GRUModel()
    m_async.load_state_dict(state)
    m_async = m_async.cuda().eval()
    m_async.stream_ordered = True
    m_sync = models.GRUModel()
    m_sync.load_state_dict(state)
    m_sync = m_sync.cuda().eval()
    assert not m_sync.stream_ordered
    x = _dev(synth.counts_windows(200, 10000, seed=7))
    with torch.inference_mode():
        m_async(x)                                # warm-up
        torch.cuda.synchronize()
        res = {}
        _assert_no_wait(lambda: res.setdefault("y", m_async(x)))
        want = m_sync(x)
        torch.cuda.synchronize()
    assert np.array_equal(res["y"].cpu().numpy(), want.cpu().numpy())
    assert m_async.engine().split()["status"] == "certified"
