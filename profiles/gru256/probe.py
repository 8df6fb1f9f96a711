"""GRU(256) throughput at 200 x 10 000 (the reference's batch of 10 000-column chunks): the engine in fp32-parity and half
precision, device-resident and host to host, beside PyTorch-ROCm's stock nn.GRU(10, 256, 2, bidirectional) + Linear + softmax
on the same GPU in the same run.  One JSON line per measurement.  Usage: python profiles/gru256/probe.py [--reps N] [--only engine]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from medaka_amd import engine, synth  # noqa: E402

H, F, L, B, T = 256, 10, 2, 200, 10000


def seeded_state(seed=0):
    rng = np.random.default_rng(seed)
    k = 1.0 / np.sqrt(H)
    st = {}
    for layer in range(L):
        kin = F if layer == 0 else 2 * H
        for sfx in ("", "_reverse"):
            st[f"gru.weight_ih_l{layer}{sfx}"] = rng.uniform(-k, k, (3 * H, kin)).astype(np.float32)
            st[f"gru.weight_hh_l{layer}{sfx}"] = rng.uniform(-k, k, (3 * H, H)).astype(np.float32)
            st[f"gru.bias_ih_l{layer}{sfx}"] = rng.uniform(-k, k, 3 * H).astype(np.float32)
            st[f"gru.bias_hh_l{layer}{sfx}"] = rng.uniform(-k, k, 3 * H).astype(np.float32)
    st["linear.weight"] = rng.uniform(-k, k, (5, 2 * H)).astype(np.float32)
    st["linear.bias"] = rng.uniform(-k, k, 5).astype(np.float32)
    return st


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts))


def emit(what, prec, med, best):
    print(json.dumps({"what": what, "precision": prec, "B": B, "T": T, "ms_median": round(1e3 * med, 2), "ms_best": round(1e3 * best, 2),
                      "Mcols_per_s": round(B * T / med / 1e6, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    st = seeded_state()
    x = synth.counts_windows(B, T, depth=40, seed=1)
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty((B, T, 5), device="cuda")
    e = engine.GruEngine(st, num_features=F, gru_size=H, n_layers=L, bidirectional=True)
    s = torch.cuda.current_stream().cuda_stream
    for half in (False, True):
        e.set_precision(half)
        prec = "half" if half else "fp32"
        emit("engine device-resident", prec, *timed(lambda: e.forward_ptr(xd.data_ptr(), B, T, yd.data_ptr(), stream=s), a.reps))
        out = np.empty((B, T, 5), np.float32)
        emit("engine host-to-host", prec, *timed(lambda: e.forward_host(x, out=out), a.reps))
    e.close()
    if a.only == "engine":
        return
    gru = torch.nn.GRU(F, H, num_layers=L, bidirectional=True, batch_first=True)
    lin = torch.nn.Linear(2 * H, 5)
    gru.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in st.items() if k.startswith("gru.")})
    lin.load_state_dict({k[7:]: torch.from_numpy(v) for k, v in st.items() if k.startswith("linear.")})
    gru, lin = gru.cuda().eval(), lin.cuda().eval()
    # MIOpen first (what nn.GRU runs on a ROCm device); where it refuses the shape, the same module with MIOpen off (ATen's
    # own cell loop) -- what a user would have to switch to
    for miopen in (True, False):
        torch.backends.cudnn.enabled = miopen
        for half in (False, True):
            g, li, xin = (gru.half(), lin.half(), xd.half()) if half else (gru.float(), lin.float(), xd)
            prec = "half" if half else "fp32"
            what = "stock nn.GRU" + ("" if miopen else " (MIOpen off)")

            def stock():
                with torch.inference_mode():
                    return torch.softmax(li(g(xin)[0]), dim=-1)

            def stock_host():
                with torch.inference_mode():
                    xi = torch.from_numpy(x).cuda()
                    return torch.softmax(li(g(xi.half() if half else xi)[0]), dim=-1).float().cpu()
            try:
                emit(what + " device-resident", prec, *timed(stock, 2))
                emit(what + " host-to-host", prec, *timed(stock_host, 2))
            except RuntimeError as err:
                torch.cuda.synchronize()
                print(json.dumps({"what": what, "precision": prec, "B": B, "T": T, "error": str(err).split("\n")[0]}), flush=True)

if __name__ == "__main__":
    main()
