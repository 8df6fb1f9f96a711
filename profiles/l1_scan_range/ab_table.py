"""Medians, spreads and ratios of the A/B runs of ab.sh: python ab_table.py <directory of the .jsonl files>."""
import json
import os
import statistics as st
import sys

out = sys.argv[1]
rows = []
for name in ("headline", "batch100", "half", "devonly", "devonly_b100", "devonly_half"):
    if not os.path.exists(f"{out}/parent_{name}.jsonl"):
        continue
    r = {t: [json.loads(l) for l in open(f"{out}/{t}_{name}.jsonl") if l.strip().startswith("{")] for t in ("parent", "new")}
    for k in ["ms_per_step"] + (["rec_l0_ms", "rec_l1_ms"] if name.startswith("devonly") else []):
        p, n = [v[k] for v in r["parent"]], [v[k] for v in r["new"]]
        rows.append({"line": name, "key": k, "parent": p, "new": n, "parent_median": st.median(p), "new_median": st.median(n),
                     "parent_spread": max(p) - min(p), "new_spread": max(n) - min(n), "gain": st.median(p) - st.median(n),
                     "ratio": st.median(n) / st.median(p)})
json.dump(rows, open(f"{out}/ab_table.json", "w"), indent=1)
for r in rows:
    print(f"{r['line']:13s} {r['key']:11s} median {r['parent_median']:.3f} -> {r['new_median']:.3f} (gain {r['gain']:.3f}, "
          f"ratio {r['ratio']:.4f}; parent spread {r['parent_spread']:.3f})")
