"""Per-kernel table of the certified async calls in a `probe.py --trace` kernel trace (rocprofv3 SQLite output).

The trace is cut wherever the GPU was idle for more than 0.2 s; a segment that holds exactly 10 `k_split_decide` dispatches
and no `k_split_audit` is one precision's 10 certified calls (probe.py leaves 0.3 s gaps around them).

    python profiles/async_forward/trace_stats.py OUT/run_results.db
"""
import collections
import re
import sqlite3
import sys


def main(path):
    c = sqlite3.connect(path)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else "kernel_name"
    rows = sorted(c.execute(f"select {name_col}, start, end from kernels").fetchall(), key=lambda r: r[1])
    segs, cur, last_end = [], [], None
    for r in rows:
        if last_end is not None and r[1] - last_end > 200_000_000:
            segs.append(cur)
            cur = []
        cur.append(r)
        last_end = r[2] if last_end is None else max(last_end, r[2])
    segs.append(cur)
    for seg in segs:
        names = [r[0] for r in seg]
        if sum("k_split_decide" in n for n in names) != 10 or any("k_split_audit" in n for n in names):
            continue
        agg = collections.defaultdict(lambda: [0, 0.0])
        for n, s, e in seg:
            short = re.sub(r"\(.*", "", n)
            agg[short][0] += 1
            agg[short][1] += (e - s) / 1e3
        span_ms = (seg[-1][2] - seg[0][1]) / 1e6
        print(f"segment: {len(seg)} dispatches, {span_ms:.2f} ms first start .. last end, {span_ms / 10:.3f} ms per call")
        print(f"{'kernel':70s} {'per call':>8s} {'avg_us':>8s} {'us per call':>11s}")
        for n, (k, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            print(f"{n[:70]:70s} {k / 10:8.1f} {t / k:8.2f} {t / 10:11.1f}")
        empty = sum(t for n, (k, t) in agg.items() if t / k < 10.0)
        print(f"launches under 10 us on average (the gated repair, the range fallbacks, decide, memsets): {empty / 10:.1f} us per call\n")


if __name__ == "__main__":
    main(sys.argv[1])
