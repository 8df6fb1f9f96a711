"""What a ragged call gains over the reference's remainder loop (prediction.py:191-209: one window per call), measured on the
device: host tensors in and out, product default settings (split scan on auto), fp32-parity and half precision.

    python profiles/ragged/measure.py [--out measure.json] [--repeats 3]

Window lists (seeded):  (a) 400 windows, lengths uniform in 1 .. 9 999;  (b) 2 000 windows, log-uniform in 50 .. 5 000;
(c) 200 windows of 9 999 columns.  For each: the loop of single-window `predict_on_batch` calls against `predict_on_ragged` at
max_cols = 1, 2 and 4 Mi columns.  One untimed pass of each variant first, then `--repeats` alternating rounds; a host clock
around calls that end in a synchronise (both entries return host tensors).  Reported: ms per list (median and the spread
max - min of the repeats) and columns/s.  The ragged results are also compared with the loop's on the sequential scan."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from medaka_amd import models, synth          # noqa: E402
from medaka_amd.torch_ext import Batch        # noqa: E402

MI = 1 << 20


def window_lists():
    rng = np.random.default_rng(20240)
    return {"a: 400 x uniform 1..9999": rng.integers(1, 10000, 400).tolist(),
            "b: 2000 x log-uniform 50..5000": np.exp(rng.uniform(np.log(50), np.log(5000), 2000)).astype(int).tolist(),
            "c: 200 x 9999": [9999] * 200}


def windows_of(lengths):
    """one long seeded pileup, cut into the windows (pinned, as the loader's batches are)"""
    pool = torch.from_numpy(synth.counts_windows(1, 20000, depth=50, seed=7)[0])
    rng = np.random.default_rng(1)
    out = []
    for n in lengths:
        s = int(rng.integers(0, 20000 - n + 1))
        out.append(pool[s:s + n].clone().pin_memory())
    return out


def loop(model, xs):
    return [model.predict_on_batch(Batch(counts_matrix=x[None]))[0] for x in xs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "measure.json"))
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device: nothing here is measured on a CPU"
    state = dict(np.load(os.path.join(ROOT, "tests", "golden", "weights_trained.npz")))
    results = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "lists": {}}
    for half in (False, True):
        model = models.GRUModel()
        model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
        model = model.to("cuda").eval()
        if half:
            model.half()
        prec = "half" if half else "fp32"
        for name, lengths in window_lists().items():
            xs = windows_of(lengths)
            cols = sum(lengths)
            variants = {"loop": lambda: loop(model, xs)}
            for mc in (1, 2, 4):
                variants[f"ragged {mc} Mi"] = (lambda mc=mc: model.predict_on_ragged(xs, max_cols=mc * MI))
            ref = None
            for v, fn in variants.items():           # untimed pass: code objects, workspace, the split scan's margin learner
                out = fn()
                if v == "loop":
                    ref = out
                else:
                    dp = max(float((a - b).abs().max()) for a, b in zip(out, ref))
                    results["lists"].setdefault(f"{name} [{prec}]", {})[f"{v}: max|dp| vs loop"] = dp
            times = {v: [] for v in variants}
            for _ in range(args.repeats):             # alternating rounds
                for v, fn in variants.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    times[v].append(1e3 * (time.perf_counter() - t0))
            row = results["lists"][f"{name} [{prec}]"]
            row["windows"], row["columns"] = len(lengths), cols
            for v, ts in times.items():
                med = statistics.median(ts)
                row[v] = {"ms": [round(t, 3) for t in ts], "median_ms": round(med, 3), "spread_ms": round(max(ts) - min(ts), 3),
                          "columns_per_s": round(cols / (med * 1e-3))}
            base = row["loop"]["median_ms"]
            print(f"{name} [{prec}]  {len(lengths)} windows, {cols} columns", flush=True)
            for v in variants:
                r = row[v]
                print(f"    {v:12s} {r['median_ms']:10.2f} ms  (spread {r['spread_ms']:.2f})  {r['columns_per_s'] / 1e6:8.2f} M columns/s  "
                      f"x{base / r['median_ms']:.2f}", flush=True)
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
        model.engine().close()


if __name__ == "__main__":
    main()
