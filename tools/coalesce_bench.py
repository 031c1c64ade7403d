"""The plain-counter coalescing, measured. Device-resident: one captured graph per leg, device
events, --rounds alternating rounds in one process. One JSON line per shape and round on stdout (and appended to
--out).

Legs (the yardsticks are the route launch and route + pack of the same run):
  route                  the route launch with the hashes written
  route+coalesce         the same launch, then sr_coalesce over its batches
  route+pack             sr_route_pack_many (the product's fused route + pack, no hashes)
  route+coalesce+pack    route launch with hashes, sr_coalesce, sr_pack_packets_many over the coalesced records
Shapes:
  c2       32 x 16 MiB of 64-byte valid metrics, 4 shards (bench.py's C2)
  c5       32 x 16 MiB of mixed 64/256/1024-byte metrics, 64 shards (bench.py's C5)
  64k      one batch of 64 KiB of C2's lines: the router's size
  same     C2's size, every line the same name
  distinct C2's size, every name distinct

    python tools/coalesce_bench.py [--rounds 3] [--iters 10] [--shapes c2,c5,64k,same,distinct] [--slots 0] [--out FILE]
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

from name_stats_bench import MIB, synthetic  # noqa: E402  (the same synthetic lines as §5.9's tables)


def shape_batches(name: str):
    """(host batches, shards)."""
    if name == "c2":
        return [pkg.gen_stream(16 * MIB, [64], seed=0x5EED0002 + 65_537 * b).data for b in range(32)], 4
    if name == "c5":
        return [pkg.gen_stream(16 * MIB, [64, 256, 1024], seed=0x5EED0005 + 65_537 * b).data for b in range(32)], 64
    if name == "64k":
        return [pkg.gen_stream(64 << 10, [64], seed=0x5EED0002).data], 4
    if name in ("same", "distinct"):
        return [synthetic(16 * MIB, name == "distinct", b) for b in range(32)], 4
    raise SystemExit(f"unknown shape {name}")


def bench_shape(name: str, rounds: int, iters: int, slots: int, emit):
    import torch

    host, shards = shape_batches(name)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), pkg.Router(shards, max(int(h.size) for h in host)) as r:
        r.set_stream(stream.cuda_stream)
        r.set_alive([1] * shards)
        r.coalesce_open(slots)
        keep, route, fused, co, pack = [], [], [], [], []
        z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device="cuda")
        for h in host:
            nb, cap = int(h.size), int(h.size) // 32 + 16   # every shape here has lines of 64 bytes or more
            mp = pkg.max_packets(nb, shards)
            d_bytes = torch.empty(nb + pkg.coalesce_append_capacity(nb), dtype=torch.uint8, device="cuda")
            d_bytes[:nb].copy_(torch.from_numpy(np.ascontiguousarray(h)))
            d_recs, d_hash, d_cout, d_srt = (torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(4))
            d_n, d_cc, d_counts = z(1, torch.int64), z(4, torch.int64), z(3, torch.int64)
            d_pd, d_pk = z((shards + 63) // 64, torch.int64), z(2 * mp, torch.int64)
            d_fin, d_fout = z(shards, torch.int16), z(shards, torch.int16)
            keep += [d_bytes, d_recs, d_hash, d_cout, d_srt, d_n, d_cc, d_counts, d_pd, d_pk, d_fin, d_fout]
            p = lambda t: t.data_ptr()
            route.append((p(d_bytes), nb, p(d_recs), cap, p(d_hash), p(d_n), p(d_pd)))
            fused.append((p(d_bytes), nb, p(d_recs), cap, None, p(d_n), p(d_pd), p(d_fin), p(d_srt), p(d_pk), mp,
                          p(d_counts), p(d_fout)))
            co.append((p(d_bytes), nb, nb, p(d_recs), p(d_n), cap, p(d_hash), p(d_cout), p(d_cc)))
            pack.append((p(d_cout), p(d_cc), cap, p(d_fin), p(d_pd), p(d_srt), p(d_pk), mp, p(d_counts), p(d_fout)))
        cb = r.coalesce_batches(co)

        def route_coalesce():
            r.route_device_many(route)
            r.coalesce(cb)

        def all_three():
            route_coalesce()
            r.pack_packets_many(pack)

        legs = {"route": lambda: r.route_device_many(route), "route+coalesce": route_coalesce,
                "route+pack": lambda: r.route_pack_many(fused), "route+coalesce+pack": all_three}
        for _ in range(2):   # warm: code loaded, layout probed, scratch allocated
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        n = len(host)
        lines = sum(int(keep[12 * i + 5][0]) for i in range(n))
        cc = np.stack([keep[12 * i + 6].cpu().numpy() for i in range(n)]).sum(axis=0)
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
            emit({"what": "coalesce", "shape": name, "round": rnd, "batches": n,
                  "bytes": int(sum(int(h.size) for h in host)), "lines": lines, "shards": shards,
                  "slots": slots or pkg.SR_COALESCE_DEFAULT_SLOTS,
                  "lines_out": int(cc[0]), "lines_dropped": int(cc[1]), "groups": int(cc[2]), "text_bytes": int(cc[3]),
                  "route_ms": round(ms["route"], 4), "route_coalesce_ms": round(ms["route+coalesce"], 4),
                  "route_pack_ms": round(ms["route+pack"], 4),
                  "route_coalesce_pack_ms": round(ms["route+coalesce+pack"], 4),
                  "coalesce_ms": round(ms["route+coalesce"] - ms["route"], 4),
                  "coalesce_over_route": round((ms["route+coalesce"] - ms["route"]) / ms["route"], 3),
                  "with_over_without": round(ms["route+coalesce+pack"] / ms["route+pack"], 3),
                  "layout": pkg.LAYOUT_NAMES.get(r.last_layout(), "?"), "iters": iters})
        del keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10, help="graph replays per timed window")
    ap.add_argument("--shapes", default="c2,c5,64k,same,distinct")
    ap.add_argument("--slots", type=int, default=0, help="table slots per batch (0: the default)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("coalesce_bench needs a GPU: nothing is measured without one")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for name in a.shapes.split(","):
        bench_shape(name, a.rounds, a.iters, a.slots, emit)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
