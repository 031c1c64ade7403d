"""The line grammar, measured. Device-resident: one captured graph per leg, device events over
--iters replays, --rounds alternating rounds in one process. One JSON line per shape and round on stdout (and
appended to --out, profiles/r17/validate.jsonl by default).

Legs (the yardsticks are the route launch and route + pack of the same run):
  route                  the route launch (no hashes)
  route+validate         the same launch, then sr_validate over its batches
  route+pack             sr_route_pack_many (the product's fused route + pack)
  route+validate+pack    route launch, sr_validate, sr_pack_packets_many over the kept records
Shapes (the configuration drops every reason but OK):
  c2        32 x 16 MiB of 64-byte valid metrics, 4 shards (bench.py's C2)
  c5        32 x 16 MiB of mixed 64/256/1024-byte metrics, 64 shards (bench.py's C5)
  64k       one batch of 64 KiB of C2's lines: the router's size
  allbad    C2's size, every line 64 bytes and failing in its last field (a space in the last tag): the whole
            line is walked and every record dropped
  tags      C5's size and shards, every line with a 200-byte tag section: the mask-only part dominates

    python tools/validate_bench.py [--rounds 3] [--iters 10] [--shapes c2,c5,64k,allbad,tags] [--out FILE]
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
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r17", "validate.jsonl")


def one_line_batches(line: bytes, nbytes: int, count: int):
    reps = nbytes // len(line)
    one = np.frombuffer(line * reps, np.uint8)
    return [one] * count


def shape(name: str):
    """(host batches, shards)."""
    if name == "c2":
        return [pkg.gen_stream(16 * MIB, [64], seed=0x5EED0002 + 65_537 * b).data for b in range(32)], 4
    if name == "c5":
        return [pkg.gen_stream(16 * MIB, [64, 256, 1024], seed=0x5EED0005 + 65_537 * b).data for b in range(32)], 64
    if name == "64k":
        return [pkg.gen_stream(64 << 10, [64], seed=0x5EED0002).data], 4
    if name == "allbad":
        line = b"svc.tenant.requests.count.padde:123456|c|@0.5|#env:prod,bad tag\n"
        assert len(line) == 64
        return one_line_batches(line, 16 * MIB, 32), 4
    if name == "tags":
        line = b"svc.tenant.requests.latency:123|ms|@0.5|#" + (b"key:value," * 20)[:200] + b"\n"
        return one_line_batches(line, 16 * MIB, 32), 64
    raise SystemExit(f"unknown shape {name}")


def bench_shape(name: str, rounds: int, iters: int, emit):
    import torch

    host, shards = shape(name)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), pkg.Router(shards, max(int(h.size) for h in host)) as r:
        r.set_stream(stream.cuda_stream)
        r.set_alive([1] * shards)
        r.validate_open(pkg.ValidateConfig(pkg.SR_VALID_DROP_ALL))
        keep, route, fused, va, pack = [], [], [], [], []
        z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device="cuda")
        for h in host:
            nb, cap = int(h.size), int(h.size) // 32 + 16   # every shape here has lines of 64 bytes or more
            mp = pkg.max_packets(nb, shards)
            d_bytes = torch.from_numpy(np.ascontiguousarray(h)).cuda()
            d_recs, d_vout, d_srt = (torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3))
            d_n, d_vc, d_counts = z(1, torch.int64), z(4, torch.int64), z(3, torch.int64)
            d_pd, d_pk = z((shards + 63) // 64, torch.int64), z(2 * mp, torch.int64)
            d_fin, d_fout = z(shards, torch.int16), z(shards, torch.int16)
            keep.append([d_bytes, d_recs, d_vout, d_srt, d_n, d_vc, d_counts, d_pd, d_pk, d_fin, d_fout])
            p = lambda t: t.data_ptr()
            route.append((p(d_bytes), nb, p(d_recs), cap, None, p(d_n), p(d_pd)))
            fused.append((p(d_bytes), nb, p(d_recs), cap, None, p(d_n), p(d_pd), p(d_fin), p(d_srt), p(d_pk), mp,
                          p(d_counts), p(d_fout)))
            va.append((p(d_bytes), nb, p(d_recs), p(d_n), cap, p(d_vout), 0, 0, 0, p(d_vc)))
            pack.append((p(d_vout), p(d_vc), cap, p(d_fin), p(d_pd), p(d_srt), p(d_pk), mp, p(d_counts), p(d_fout)))
        vb = r.validate_batches(va)

        def route_validate():
            r.route_device_many(route)
            r.validate(vb)

        def all_three():
            route_validate()
            r.pack_packets_many(pack)

        legs = {"route": lambda: r.route_device_many(route), "route+validate": route_validate,
                "route+pack": lambda: r.route_pack_many(fused), "route+validate+pack": all_three}
        for _ in range(2):   # warm: code loaded, layout probed, scratch allocated
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        n = len(host)
        lines = sum(int(k[4][0]) for k in keep)
        vc = np.stack([k[5].cpu().numpy() for k in keep]).sum(axis=0)
        r.validate_reset()
        route_validate()
        hits = r.validate_read()
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
            emit({"what": "validate", "shape": name, "round": rnd, "batches": n,
                  "bytes": int(sum(int(h.size) for h in host)), "lines": lines, "shards": shards,
                  "lines_out": int(vc[0]), "lines_dropped": int(vc[1]), "bytes_dropped": int(vc[2]), "subject": int(vc[3]),
                  "reasons": {pkg.validate_reason_name(q): int(hits[q, 0]) for q in range(len(hits)) if int(hits[q, 0])},
                  "route_ms": round(ms["route"], 4), "route_validate_ms": round(ms["route+validate"], 4),
                  "route_pack_ms": round(ms["route+pack"], 4), "route_validate_pack_ms": round(ms["route+validate+pack"], 4),
                  "validate_ms": round(ms["route+validate"] - ms["route"], 4),
                  "route_validate_over_route": round(ms["route+validate"] / ms["route"], 3),
                  "with_over_without": round(ms["route+validate+pack"] / ms["route+pack"], 3),
                  "layout": pkg.LAYOUT_NAMES.get(r.last_layout(), "?"), "iters": iters})
        del keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10, help="graph replays per timed window")
    ap.add_argument("--shapes", default="c2,c5,64k,allbad,tags")
    ap.add_argument("--out", default=DEFAULT_OUT, help="append the JSON lines to this file too")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("validate_bench needs a GPU: nothing is measured without one")

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
