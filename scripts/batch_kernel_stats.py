"""profiles/batch_kernel_stats.csv from the kernel trace of  rocprofv3 --kernel-trace --stats -d DIR -o batch -- python
scripts/batch_bench.py --lanes 8 --reps 10  (rocprofv3 writes DIR/batch_results.db, an SQLite file with a `kernels` view).

  python scripts/batch_kernel_stats.py DIR/batch_results.db [profiles/batch_kernel_stats.csv]

Two tables: per kernel name (calls, total, average, share, min, max, median of the launch durations in ns), then "PerGrid": the
pass and solver launches per grid shape - blocks in x (k_lm_solve_batch: live lanes), lanes in y - with the median, p10 and p90 of
their durations and the scratch size the trace reports.  A launch whose lanes are all done returns at once: such launches are in
the counts (they pull p10 down), which is why the medians are quoted."""
import collections
import csv
import sqlite3
import sys

import numpy as np


def main():
    db = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else "profiles/batch_kernel_stats.csv"
    rows = sqlite3.connect(db).execute("select name, duration, grid_x, grid_y, workgroup_x, scratch_size from kernels").fetchall()
    total = sum(r[1] for r in rows)
    by_name = collections.defaultdict(list)
    by_grid = collections.defaultdict(list)
    scratch = {}
    for name, d, gx, gy, wx, sc in rows:
        by_name[name].append(d)
        if "k_gicp_pass" in name or "k_lm_solve" in name:
            key = (name.split("(")[0], gx // wx, gy)  # (grid_x is in threads)
            by_grid[key].append(d)
            scratch[key] = sc
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs", "MedianNs"])
        for name, ds in sorted(by_name.items(), key=lambda kv: -sum(kv[1])):
            w.writerow([name, len(ds), sum(ds), round(sum(ds) / len(ds), 1), round(100 * sum(ds) / total, 3), min(ds), max(ds), int(np.median(ds))])
        w.writerow([])
        w.writerow(["PerGrid: Name", "blocks_x (k_lm_solve_batch: live lanes)", "lanes_y", "Calls", "MedianNs", "P10Ns", "P90Ns", "ScratchBytes"])
        for key, ds in sorted(by_grid.items()):
            ds = np.array(ds)
            w.writerow([key[0], key[1], key[2], len(ds), int(np.median(ds)), int(np.percentile(ds, 10)), int(np.percentile(ds, 90)), scratch[key]])


if __name__ == "__main__":
    main()
