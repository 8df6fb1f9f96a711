import os, sys, time
os.environ.pop("MDK_SCAN_SPLIT", None)
os.environ["MDK_SCAN_SPLIT_ADAPT"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # the repository root; run from there
import numpy as np, torch
from medaka_amd import engine, synth
gold = dict(np.load("tests/golden/weights_trained.npz"))
cases = [(200, 10000, False), (100, 10000, False), (37, 9999, False), (200, 10000, True)]
if len(sys.argv) > 1:
    cases = cases[:int(sys.argv[1])]
for B, T, half in cases:
    x = synth.counts_windows(B, T, depth=40, seed=7 * B + T)
    xd = torch.from_numpy(x).cuda()
    outs = {}
    plan = engine.split_plan(B, T)
    for lvl in (0, 1, 2):
        e = engine.GruEngine(gold)
        e.set_precision(half)
        e.set_option("scan_split_trim", lvl)
        e.enable_timing(True)
        yd = torch.empty(B, T, 5, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        e.forward_ptr(xd.data_ptr(), B, T, yd.data_ptr(), stream=st); torch.cuda.synchronize()
        info = e.split()
        rec = []
        for _ in range(5):
            e.forward_ptr(xd.data_ptr(), B, T, yd.data_ptr(), stream=st); torch.cuda.synchronize()
            rec.append(e.timing()["rec_ms"] + [e.timing()["total_ms"]])
        rec = np.median(np.array(rec), axis=0)
        out = yd.cpu().numpy()
        host = e.forward_host(x)
        t = e.timing()
        print(f"B={B} T={T} half={half} trim={lvl}: {info['status']} chunks {info['chunks']} margin {info['margin']} fallbacks {info['fallbacks']} "
              f"max_delta {info['max_delta']:.3e} audit {info['audit_max_dp']:.3e}; rec_ms l0 {rec[0]:.3f} l1 {rec[1]:.3f} total {rec[2]:.3f}; "
              f"host==dev {np.array_equal(host, out)} launches {t['rec_launches']} streamed {t['host_streamed']}", flush=True)
        outs[lvl] = out
        e.close()
    d1 = outs[1] != outs[0]
    print(f"   trim 1 vs 0: identical {not d1.any()}, differing values {int(d1.sum())}, max|dp| {np.abs(outs[1]-outs[0]).max():.3e}")
    if d1.any():
        cols = np.nonzero(d1.any(axis=(0, 2)))[0]
        per = [int(((cols >= plan['first'][k]) & (cols < plan['last'][k])).sum()) for k in range(plan['chunks'])]
        print(f"   differing columns per chunk: {per}; first {cols[:5]}, last {cols[-5:]}")
    d2 = np.abs(outs[2] - outs[0])
    print(f"   trim 2 vs 0: max|dp| {d2.max():.3e}, argmax identical {np.array_equal(outs[2].argmax(-1), outs[0].argmax(-1))}", flush=True)
