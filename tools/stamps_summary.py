#!/usr/bin/env python3
"""The record-base chain out of tools/stamps_route's raw dump (stamps_raw.bin: per tile
workgroup the s_memrealtime stamps entry, 0, 6, exit, HW_ID, XCC_ID, 3, 7, 1, 13, 12, 4 and, from the
13-column dumps on, 15; 100 MHz ticks). Prints one JSON object of percentiles (p10, p50, p90, p99, in µs):

  landed_to_published   stamp 0 -> 1: wave 0 has its bytes -> the tile's count granule is stored
  published_to_ring     stamp 1 -> 13: ... -> the scanner has the tile's base in its ring
  published_to_base     stamp 1 -> 12: ... -> the scanner's publisher has stored the tile's base granule
  landed_to_base        stamp 0 -> 12
  landed_to_first_rec   stamp 0 -> 3: ... -> the tile reaches its first record store
  base_before_first_rec stamp 12 -> 3 (negative: the base was stored after the tile asked for it)
  wait_at_first_record  stamp 3 -> 7
  lifetime              stamp 0 -> 6

  python tools/stamps_summary.py stamps_raw.bin [--cols 12] [--out summary.json]
"""
import argparse
import json

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("raw")
    ap.add_argument("--cols", type=int, default=13, help="12 for dumps without stamp 15")
    ap.add_argument("--out")
    a = ap.parse_args()
    d = np.fromfile(a.raw, dtype=np.uint64).reshape(-1, a.cols).astype(np.int64)
    s0, s6, s3, s7, s1, s13, s12 = d[:, 1], d[:, 2], d[:, 6], d[:, 7], d[:, 8], d[:, 9], d[:, 10]
    ok = (s0 > 0) & (s1 > 0)

    def pc(x):
        return [round(float(v) * 0.01, 2) for v in np.percentile(x, [10, 50, 90, 99])] if x.size else None

    w = ok & (s3 > 0)
    b = ok & (s12 > 0)
    res = {
        "tiles": int(ok.sum()),
        "percentiles": [10, 50, 90, 99],
        "landed_to_published": pc((s1 - s0)[ok]),
        "published_to_ring": pc((s13 - s1)[ok & (s13 > 0)]),
        "published_to_base": pc((s12 - s1)[b]),
        "landed_to_base": pc((s12 - s0)[b]),
        "landed_to_first_rec": pc((s3 - s0)[w]),
        "base_before_first_rec": pc((s3 - s12)[w & b]),
        "base_stored_after_first_rec_frac": round(float(((s12 > s3) & w & b).sum()) / max(int((w & b).sum()), 1), 4),
        "wait_at_first_record": pc((s7 - s3)[w]),
        "lifetime": pc((s6 - s0)[ok]),
    }
    if a.cols > 12:
        s15 = d[:, 12]
        res["landed_to_image_complete"] = pc((s15 - s0)[ok & (s15 > 0)])
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
