"""The name rules, measured. Device-resident: one captured graph per leg, device events over
--iters replays, --rounds alternating rounds in one process. One JSON line per shape and round on stdout (and
appended to --out).

Legs (the yardsticks are the route launch and route + pack of the same run):
  route               the route launch (no hashes)
  route+rules         the same launch, then sr_rules over its batches
  route+pack          sr_route_pack_many (the product's fused route + pack)
  route+rules+pack    route launch, sr_rules, sr_pack_packets_many over the kept records
Shapes:
  c2        32 x 16 MiB of 64-byte valid metrics, 4 shards (bench.py's C2), a small block list
  c5        32 x 16 MiB of mixed 64/256/1024-byte metrics, 64 shards (bench.py's C5), the same list
  64k       one batch of 64 KiB of C2's lines: the router's size
  onerule   C2's size, every line matching one 64-byte DROP rule
  nomatch   C2's size, 256 rules of which none matches (none shares a first byte with a line: the first-byte
            filter alone is measured)
  nearmiss  C2's size, 256 rules of which none matches, each the first 11 bytes of a line of the traffic and a
            byte that no line holds: every line passes the filter, fetches a second step and runs the search

    python tools/rules_bench.py [--rounds 3] [--iters 10] [--shapes c2,c5,64k,onerule,nomatch,nearmiss] [--out FILE]
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
P, X, D, K = pkg.SR_RULE_PREFIX, pkg.SR_RULE_EXACT, pkg.SR_RULE_DROP, pkg.SR_RULE_KEEP


def block_list(host):
    """A small block list taken from the traffic itself: the first line's name exactly, the second line's first
    four bytes as a prefix with an exception for its first eight, and rules that match nothing."""
    first = bytes(host[0][:8192]).split(b"\n")
    n0, n1 = first[0].split(b":")[0][:64], first[1].split(b":")[0][:64]
    rules = [(n0, X, D), (n1[:4], P, D), (n1[:8], P, K), (b"debug.", P, D), (b"tmp.", P, D)]
    return [r for i, r in enumerate(rules) if r[0] and (r[0], r[1]) not in {(q[0], q[1]) for q in rules[:i]}]


def one_line_batches(line: bytes, nbytes: int, count: int):
    reps = nbytes // len(line)
    one = np.frombuffer(line * reps, np.uint8)
    return [one] * count


def shape(name: str):
    """(host batches, shards, rules)."""
    if name == "c2":
        host = [pkg.gen_stream(16 * MIB, [64], seed=0x5EED0002 + 65_537 * b).data for b in range(32)]
        return host, 4, block_list(host)
    if name == "c5":
        host = [pkg.gen_stream(16 * MIB, [64, 256, 1024], seed=0x5EED0005 + 65_537 * b).data for b in range(32)]
        return host, 64, block_list(host)
    if name == "64k":
        host = [pkg.gen_stream(64 << 10, [64], seed=0x5EED0002).data]
        return host, 4, block_list(host)
    if name == "onerule":   # a 64-byte name: lines of 70 bytes
        pat = (b"tenant.blocked.metric.name.padded.to.sixty.four.bytes" + b"." * 64)[:64]
        return one_line_batches(pat + b":1|c\n", 16 * MIB, 32), 4, [(pat, X, D)]
    if name == "nomatch":   # C2's lines; 256 rules of 16 bytes that begin with bytes no statsd name here begins with
        host = [pkg.gen_stream(16 * MIB, [64], seed=0x5EED0002 + 65_537 * b).data for b in range(32)]
        return host, 4, [(bytes([(1 + i % 31) if i % 31 != 9 else 127]) + b"%03d.never.match" % i, P, D) for i in range(256)]   # no '\n'
    if name == "nearmiss":
        host = [pkg.gen_stream(16 * MIB, [64], seed=0x5EED0002 + 65_537 * b).data for b in range(32)]
        heads = []
        for l in bytes(host[0][:1 << 20]).split(b"\n"):
            h = l[:11]
            if len(l) > 20 and b":" not in h and h not in heads:
                heads.append(h)
            if len(heads) == 256:
                break
        return host, 4, [(h + b"\x01neve", P, D) for h in heads]
    raise SystemExit(f"unknown shape {name}")


def bench_shape(name: str, rounds: int, iters: int, emit):
    import torch

    host, shards, rules = shape(name)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), pkg.Router(shards, max(int(h.size) for h in host)) as r:
        r.set_stream(stream.cuda_stream)
        r.set_alive([1] * shards)
        r.rules_open(pkg.RuleSet(rules))
        keep, route, fused, ru, pack = [], [], [], [], []
        z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device="cuda")
        for h in host:
            nb, cap = int(h.size), int(h.size) // 32 + 16   # every shape here has lines of 64 bytes or more
            mp = pkg.max_packets(nb, shards)
            d_bytes = torch.from_numpy(np.ascontiguousarray(h)).cuda()
            d_recs, d_rout, d_srt = (torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3))
            d_n, d_rc, d_counts = z(1, torch.int64), z(4, torch.int64), z(3, torch.int64)
            d_pd, d_pk = z((shards + 63) // 64, torch.int64), z(2 * mp, torch.int64)
            d_fin, d_fout = z(shards, torch.int16), z(shards, torch.int16)
            keep.append([d_bytes, d_recs, d_rout, d_srt, d_n, d_rc, d_counts, d_pd, d_pk, d_fin, d_fout])
            p = lambda t: t.data_ptr()
            route.append((p(d_bytes), nb, p(d_recs), cap, None, p(d_n), p(d_pd)))
            fused.append((p(d_bytes), nb, p(d_recs), cap, None, p(d_n), p(d_pd), p(d_fin), p(d_srt), p(d_pk), mp,
                          p(d_counts), p(d_fout)))
            ru.append((p(d_bytes), nb, p(d_recs), p(d_n), cap, p(d_rout), 0, 0, 0, p(d_rc)))
            pack.append((p(d_rout), p(d_rc), cap, p(d_fin), p(d_pd), p(d_srt), p(d_pk), mp, p(d_counts), p(d_fout)))
        rb = r.rules_batches(ru)

        def route_rules():
            r.route_device_many(route)
            r.rules(rb)

        def all_three():
            route_rules()
            r.pack_packets_many(pack)

        legs = {"route": lambda: r.route_device_many(route), "route+rules": route_rules,
                "route+pack": lambda: r.route_pack_many(fused), "route+rules+pack": all_three}
        for _ in range(2):   # warm: code loaded, layout probed, scratch allocated
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        n = len(host)
        lines = sum(int(k[4][0]) for k in keep)
        rc = np.stack([k[5].cpu().numpy() for k in keep]).sum(axis=0)
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
            emit({"what": "rules", "shape": name, "round": rnd, "batches": n,
                  "bytes": int(sum(int(h.size) for h in host)), "lines": lines, "shards": shards, "rules": len(rules),
                  "lines_out": int(rc[0]), "lines_dropped": int(rc[1]), "bytes_dropped": int(rc[2]), "subject": int(rc[3]),
                  "route_ms": round(ms["route"], 4), "route_rules_ms": round(ms["route+rules"], 4),
                  "route_pack_ms": round(ms["route+pack"], 4), "route_rules_pack_ms": round(ms["route+rules+pack"], 4),
                  "rules_ms": round(ms["route+rules"] - ms["route"], 4),
                  "route_rules_over_route": round(ms["route+rules"] / ms["route"], 3),
                  "with_over_without": round(ms["route+rules+pack"] / ms["route+pack"], 3),
                  "layout": pkg.LAYOUT_NAMES.get(r.last_layout(), "?"), "iters": iters})
        del keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10, help="graph replays per timed window")
    ap.add_argument("--shapes", default="c2,c5,64k,onerule,nomatch,nearmiss")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("rules_bench needs a GPU: nothing is measured without one")

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
