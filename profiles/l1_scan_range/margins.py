"""Margin learner per weight set at scan_split_trim 0 and 2 (200 x 10000, i.i.d. 50x pileups), and the forced-margin table."""
import json, os, sys
os.environ.pop("MDK_SCAN_SPLIT", None)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # the repository root; run from there
import numpy as np, torch
from medaka_amd import engine, synth
gold = dict(np.load("tests/golden/weights_trained.npz"))
z = np.load("tests/golden/weights_zoo.npz")
names = ["trained"] + sorted({k.split("/")[0] for k in z.files})
def weights(n):
    return gold if n == "trained" else {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")}
B, T = 200, 10000
x = np.concatenate([synth.counts_windows(8, T, depth=50, seed=100 + s) for s in range(25)])
xd = torch.from_numpy(x).cuda()
yd = torch.empty(B, T, 5, device="cuda")
st = torch.cuda.current_stream().cuda_stream
res = {}
for n in names:
    res[n] = {}
    for lvl in (0, 1, 2):
        e = engine.GruEngine(weights(n))
        e.set_option("scan_split_trim", lvl)
        e.set_option("scan_split", 0)
        e.forward_ptr(xd.data_ptr(), B, T, yd.data_ptr(), stream=st); torch.cuda.synchronize()
        seq = yd.cpu().numpy()
        e.set_option("scan_split", 1)
        margins, worst_dp, deltas = [], 0.0, []
        for i in range(30):
            e.forward_ptr(xd.data_ptr(), B, T, yd.data_ptr(), stream=st); torch.cuda.synchronize()
            info = e.split()
            margins.append(info["margin"] if info["chunks"] > 1 and info["status"] == "certified" else 0)
            deltas.append(info["max_delta"])
            if i in (0, 29) or margins[-1] != (margins[-2] if len(margins) > 1 else None):
                worst_dp = max(worst_dp, float(np.abs(yd.cpu().numpy() - seq).max()))
        out = yd.cpu().numpy()
        row = {"margins_over_30_calls": margins, "settled_at": margins[-1], "status": info["status"], "rejected_certificates": info["fallbacks"],
               "max_junction_delta_settled": info["max_delta"], "largest_junction_delta_of_a_certified_call": max([d for d, m in zip(deltas, margins) if m] or [0.0]),
               "audits": info["audits"], "audit_failures": info["audit_failures"], "audit_worst_dp": info["audit_worst_dp"],
               "max_dp_vs_sequential": worst_dp, "argmax_identical": bool(np.array_equal(out.argmax(-1), seq.argmax(-1)))}
        # forced margins (a rejection is answered sequentially, not escalated)
        forced = {}
        e2 = engine.GruEngine(weights(n))
        e2.set_option("scan_split_trim", lvl)
        e2.set_option("scan_split_audit", 0)
        for g in (64, 96, 128, 192, 256):
            e2.set_option("scan_split_margin", g)
            e2.set_option("scan_split", 5)
            e2.forward_ptr(xd.data_ptr(), B, T, yd.data_ptr(), stream=st); torch.cuda.synchronize()
            i2 = e2.split()
            forced[g] = {"status": i2["status"], "max_junction_delta": i2["max_delta"], "max_dp_vs_sequential": float(np.abs(yd.cpu().numpy() - seq).max())}
        e2.close()
        row["forced_margins"] = forced
        res[n][f"trim{lvl}"] = row
        print(n, f"trim {lvl}: settles at {row['settled_at']} ({row['status']}, {row['rejected_certificates']} rejected), delta {row['max_junction_delta_settled']:.2e}, "
              f"audit worst {row['audit_worst_dp']:.2e}, max|dp| vs seq {worst_dp:.2e}; forced: " +
              ", ".join(f"{g}:{r['status'][:4]}({r['max_junction_delta']:.1e})" for g, r in forced.items()), flush=True)
        e.close()
json.dump(res, open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "margins.json"), "w"), indent=1)
