"""The name statistics, measured. Device-resident: one captured graph per leg, device events,
--rounds alternating rounds in one process. One JSON line per leg and round on stdout (and appended to --out).

Shapes (each with the leg `route`: the route launch with the hashes written, alone, which is the yardstick of
the same run, and the leg `route+stats`: the same launch followed by sr_stats_update over its batches):
  c2       32 x 16 MiB of 64-byte valid metrics, 4 shards (bench.py's C2)
  c5       32 x 16 MiB of mixed 64/256/1024-byte metrics, 64 shards (bench.py's C5)
  64k, 1m  one batch of 64 KiB / 1 MiB of C2's lines: the router's sizes
  same     C2's size, every line the same name
  distinct C2's size, every name distinct
The statistics are in their steady state when timed (registers settled, hot names in the table): the update
runs several times before the first timed replay.

    python tools/name_stats_bench.py [--rounds 3] [--iters 10] [--shapes c2,c5,64k,1m,same,distinct] [--out FILE]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("statsd-router_amd")

MIB = 1 << 20


def synthetic(nbytes: int, distinct: bool, seed: int) -> np.ndarray:
    """64-byte lines "n<15 digits>....:1|c\\n"; the digits count up (distinct) or stay (same name)."""
    n = nbytes // 64
    a = np.full((n, 64), ord("x"), dtype=np.uint8)
    a[:, 0] = ord("n")
    ids = (np.arange(n, dtype=np.uint64) + np.uint64(seed * n)) if distinct else np.full(n, 7, dtype=np.uint64)
    for k in range(15):
        a[:, 15 - k] = (ids % np.uint64(10)).astype(np.uint8) + ord("0")
        ids //= np.uint64(10)
    a[:, 59:64] = np.frombuffer(b":1|c\n", dtype=np.uint8)
    return a.reshape(-1)


def shape_batches(name: str):
    """(host batches, shards)."""
    if name == "c2":
        return [pkg.gen_stream(16 * MIB, [64], seed=0x5EED0002 + 65_537 * b).data for b in range(32)], 4
    if name == "c5":
        return [pkg.gen_stream(16 * MIB, [64, 256, 1024], seed=0x5EED0005 + 65_537 * b).data for b in range(32)], 64
    if name in ("64k", "1m"):
        return [pkg.gen_stream(64 << 10 if name == "64k" else MIB, [64], seed=0x5EED0002).data], 4
    if name in ("same", "distinct"):
        return [synthetic(16 * MIB, name == "distinct", b) for b in range(32)], 4
    raise SystemExit(f"unknown shape {name}")


def bench_shape(name: str, rounds: int, iters: int, emit):
    import torch

    host, shards = shape_batches(name)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), pkg.Router(shards, max(int(h.size) for h in host)) as r:
        r.set_stream(stream.cuda_stream)
        r.set_alive([1] * shards)
        r.stats_open()
        keep, route, stats = [], [], []
        for h in host:
            nb, cap = int(h.size), int(h.size) // 32 + 16   # every shape here has lines of 64 bytes or more
            d_bytes = torch.from_numpy(np.ascontiguousarray(h)).cuda()
            d_recs = torch.empty(cap, dtype=torch.int64, device="cuda")
            d_hash = torch.empty(cap, dtype=torch.int64, device="cuda")
            d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
            keep += [d_bytes, d_recs, d_hash, d_n]
            route.append((d_bytes.data_ptr(), nb, d_recs.data_ptr(), cap, d_hash.data_ptr(), d_n.data_ptr()))
            stats.append((d_bytes.data_ptr(), nb, d_recs.data_ptr(), d_n.data_ptr(), cap, d_hash.data_ptr()))
        sb = r.stats_batches(stats)

        def both():
            r.route_device_many(route)
            r.stats_update(sb)

        legs = {"route": lambda: r.route_device_many(route), "route+stats": both}
        for _ in range(3):   # warm: code loaded, layout probed, registers settled, hot names inserted
            both()
        torch.cuda.synchronize()
        lines = sum(int(keep[4 * i + 3][0]) for i in range(len(host)))
        snap = r.stats_read()
        graphs = {}
        for leg, fn in legs.items():
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                fn()
            graphs[leg] = g
        for rnd in range(rounds):
            ms = {}
            for leg, g in graphs.items():
                g.replay()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    g.replay()
                e1.record()
                e1.synchronize()
                ms[leg] = e0.elapsed_time(e1) / iters
            emit({"what": "name_stats", "shape": name, "round": rnd, "batches": len(host),
                  "bytes": int(sum(int(h.size) for h in host)), "lines": lines, "shards": shards,
                  "hot_names": int(snap.n_hot), "names_estimate": round(pkg.stats_cardinality(snap)),
                  "route_ms": round(ms["route"], 4), "route_stats_ms": round(ms["route+stats"], 4),
                  "stats_ms": round(ms["route+stats"] - ms["route"], 4),
                  "stats_over_route": round((ms["route+stats"] - ms["route"]) / ms["route"], 3),
                  "layout": pkg.LAYOUT_NAMES.get(r.last_layout(), "?"), "iters": iters})
        del keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10, help="graph replays per timed window")
    ap.add_argument("--shapes", default="c2,c5,64k,1m,same,distinct")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("name_stats_bench needs a GPU: nothing is measured without one")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for name in a.shapes.split(","):
        bench_shape(name, a.rounds, a.iters, emit)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
