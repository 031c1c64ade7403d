#!/usr/bin/env python3
"""Per-kernel times out of a `rocprofv3 --kernel-trace` run: reads the run's *_kernel_trace.csv files
(columns Kernel_Name, Start_Timestamp, End_Timestamp, nanoseconds) and writes one JSON object, a key per
kernel name (cut at 90 characters): calls, the calls longer than --over microseconds, their median and
minimum, and the longest call. The threshold separates a kernel's big launches from its small ones (the
pull of a 273 MB group from the pulls of the sizes' all-to-all and of 4 KiB groups).

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/local_exchange_bench.py ...
  python tools/kernel_trace_summary.py DIR [--over 40] [--out profiles/r10/local_pull_kernel_trace.json]
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics


def summarise(paths, over_us):
    times = {}
    for path in paths:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
                times.setdefault(row["Kernel_Name"][:90], []).append(us)
    out = {}
    for name, us in times.items():
        big = [x for x in us if x > over_us]
        key = f"over_{over_us:g}us"
        out[name] = {
            "calls": len(us),
            f"calls_{key}": len(big),
            f"median_us_{key}": statistics.median(big) if big else None,
            f"min_us_{key}": min(big) if big else None,
            "max_us": max(us),
        }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir", help="rocprofv3's output directory (searched recursively)")
    ap.add_argument("--over", type=float, default=40.0, help="microseconds: the launches that count as big")
    ap.add_argument("--out")
    args = ap.parse_args()
    paths = sorted(glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True))
    if not paths:
        raise SystemExit(f"no *kernel_trace.csv under {args.dir}")
    text = json.dumps(summarise(paths, args.over), indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
