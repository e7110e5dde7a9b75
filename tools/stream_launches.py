#!/usr/bin/env python3
"""Kernel launches of one stream from two rocprofv3 --stats directories of `tools/stream_latency.py --trace-streams K`
(K = k1 and k2): per kernel, (calls2 - calls1) / (k2 - k1) launches per stream and their mean duration.

    python tools/stream_launches.py DIR1 k1 DIR2 k2 [steps]
"""
import csv
import glob
import json
import os
import sys


def load(d):
    fs = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not fs:
        sys.exit(f"no kernel_stats.csv under {d}")
    return {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(fs[0]))}


d1, k1, d2, k2 = sys.argv[1], int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
steps = int(sys.argv[5]) if len(sys.argv) > 5 else 1
a, b = load(d1), load(d2)
rows, total, total_us = [], 0.0, 0.0
for name, (c2, t2) in sorted(b.items(), key=lambda kv: -kv[1][1]):
    c1, t1 = a.get(name, (0, 0.0))
    if c2 == c1:
        continue
    n = (c2 - c1) / (k2 - k1)
    us = (t2 - t1) / (c2 - c1) / 1e3
    rows.append({"kernel": name.split("(")[0][:80], "per_stream": n, "per_step": round(n / steps, 2),
                 "mean_us": round(us, 2)})
    total += n
    total_us += n * us
print(json.dumps({"launches_per_stream": total, "launches_per_step": round(total / steps, 1),
                  "kernel_ms_per_stream": round(total_us / 1e3, 3), "kernels": rows}, indent=1))
