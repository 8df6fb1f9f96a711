"""The stream-ordered device forward at BASELINE configs[1] (200 x 10 000, trained weights, fp32 and half): device rate of
30 calls enqueued back to back against the synchronous device entry's 30 calls, and (--trace) a run of certified calls to
put under `rocprofv3 --kernel-trace --stats` for the cost of the decide kernel and the empty repair launches.

    python profiles/async_forward/probe.py                 # memory of a first call per entry; the rates, one JSON line per precision
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python profiles/async_forward/probe.py --trace
    python profiles/async_forward/trace_stats.py OUT/run_results.db
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("MDK_SCAN_SPLIT_ADAPT", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402

from medaka_amd import engine, synth  # noqa: E402

B, T, N = 200, 10000, 30


def rate(fn, x, out):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    h0 = time.perf_counter()
    a.record()
    for _ in range(N):
        fn(x.data_ptr(), B, T, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    h1 = time.perf_counter()
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b)
    return {"device_ms_per_call": ms / N, "columns_per_s": B * T * N / (ms * 1e-3), "host_ms_to_enqueue_all": (h1 - h0) * 1e3}


def footprint(state, x, out):
    """Device memory a fresh engine holds after its first call, one engine per entry (fp32)."""
    res = {}
    for name in ("forward_ptr", "forward_async_ptr"):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        e = engine.GruEngine(state)
        getattr(e, name)(x.data_ptr(), B, T, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        e.split()
        torch.cuda.synchronize()
        res[name + "_gb"] = round((free0 - torch.cuda.mem_get_info()[0]) / 1e9, 2)
        e.close()
    return res


def main():
    state = dict(np.load(os.path.join(ROOT, "tests", "golden", "weights_trained.npz")))
    x = torch.from_numpy(synth.counts_windows(B, T, seed=1)).cuda()
    out = torch.empty((B, T, 5), dtype=torch.float32, device="cuda")
    if "--trace" not in sys.argv:
        print(json.dumps({"device_memory_after_first_call": footprint(state, x, out)}))
    for half in (False, True):
        e = engine.GruEngine(state)
        e.set_precision(half)
        for _ in range(3):                       # workspace, probe, first audit
            e.forward_async_ptr(x.data_ptr(), B, T, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
            if "--trace" not in sys.argv:
                e.forward_ptr(x.data_ptr(), B, T, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        if "--trace" in sys.argv:
            # only the async entry in the traced part, and a 0.3 s idle gap on either side of the 10 certified calls: trace_stats.py
            # cuts the trace at those gaps and keeps the segments that hold 10 decisions and no audit
            time.sleep(0.3)
            for _ in range(10):
                e.forward_async_ptr(x.data_ptr(), B, T, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            time.sleep(0.3)
            print(json.dumps({"half": half, "split": e.split()}))
        else:
            r_async = rate(e.forward_async_ptr, x, out)
            info = e.split()
            r_sync = rate(e.forward_ptr, x, out)
            print(json.dumps({"half": half, "B": B, "T": T, "calls": N, "async": r_async, "sync": r_sync,
                              "split": {k: info[k] for k in ("status", "chunks", "margin", "fallbacks", "audits", "probes")}}))
        e.close()


if __name__ == "__main__":
    main()
