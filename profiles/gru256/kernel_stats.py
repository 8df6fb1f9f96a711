"""Per-kernel totals from the rocprofv3 database of `rocprofv3 --kernel-trace --stats -d OUT -o gru256 -- python
profiles/gru256/probe.py --reps 2 --only engine` (OUT/gru256_results.db): calls, total / average ms, per symbol.
Usage: python profiles/gru256/kernel_stats.py OUT/gru256_results.db"""
import sqlite3
import sys

c = sqlite3.connect(sys.argv[1])
cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
name = "kernel_name" if "kernel_name" in cols else "name"
rows = c.execute(f"select {name}, count(*), sum(end - start) / 1e6, avg(end - start) / 1e6 from kernels group by {name} "
                 "order by 3 desc").fetchall()
print(f"{'calls':>6} {'total ms':>10} {'avg ms':>9}  kernel")
for n, k, tot, avg in rows:
    print(f"{k:6d} {tot:10.2f} {avg:9.3f}  {n[:150]}")
