#!/usr/bin/env python3
"""sr_owner_pack against sr_pack_packets + sr_pack_payloads called directly on the same receive buffer,
and sr_flush_pending, on one GPU at world = 1.

C5's launch shape (32 batches of 16 MiB, mixed lengths, 64 shards, every shard alive) is routed and
regrouped once (sr_pack_many_by_owner with one owner: at world 1 the pack's output is the receive buffer).
Then, in one process, three rounds alternate
  direct : sr_pack_packets + sr_pack_payloads on the receive buffer, the line total in a device u64;
  owner  : sr_owner_pack on the same buffers (a zero bitmap row, so the fold does all its work): the same
           kernels plus owner_fold_kernel;
  flush  : sr_flush_pending of 64 full pending slots (and the 128-byte copy that refills the fills),
each one captured graph, timed with events around back-to-back replays after a warm-up. The two packing
legs must write identical outputs (checked before timing). One JSON line on stdout and, with --out, in a
file.

  python tools/owner_pack_bench.py [--config c5] [--reps 20] [--rounds 3] [--out FILE]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def timed(fn, reps, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def run(pkg, torch, cfg, reps, rounds):
    from bench import CONFIGS

    desc, batch_bytes, lens, p_inv, shards, seed0, _ = CONFIGS[cfg]
    M = pkg.SR_MAX_BATCHES_PER_LAUNCH
    dev = torch.device("cuda", 0)
    host = [pkg.gen_stream(batch_bytes, lens, seed=seed0 + 65_537 * b, p_invalid=p_inv) for b in range(M)]
    sizes = [int(s.data.size) for s in host]
    max_lines = max(int(s.n_lines) for s in host)
    stream = torch.cuda.Stream(device=dev)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    with torch.cuda.stream(stream), pkg.Router(shards, batch_bytes, device=0) as r:
        r.set_stream(stream.cuda_stream)
        d_in = torch.empty((M, batch_bytes), dtype=torch.uint8, device=dev)
        for b, s in enumerate(host):
            d_in[b, : sizes[b]].copy_(torch.from_numpy(s.data))
        rec, cnt = torch.empty((M, max_lines), dtype=torch.int64, device=dev), z(M, torch.int64)
        r.route_device_many([(d_in[b].data_ptr(), sizes[b], rec[b].data_ptr(), max_lines, None, cnt[b].data_ptr())
                             for b in range(M)])
        # the regroup, one owner: the receive buffer
        ocap = pkg.pack_capacity(sum(sizes))
        rb = torch.empty(ocap, dtype=torch.uint8, device=dev)
        rr = torch.empty(M * max_lines, dtype=torch.int64, device=dev)
        rc = z((1, 2), torch.int64)
        r.pack_many_by_owner([(d_in[b].data_ptr(), sizes[b], rec[b].data_ptr(), max_lines, cnt[b].data_ptr())
                              for b in range(M)], 1, rb.data_ptr(), ocap, rr.data_ptr(), rc.data_ptr())
        stream.synchronize()
        n_lines, n_bytes = (int(x) for x in rc[0].tolist())
        del d_in, rec
        mp = pkg.max_packets(n_bytes, shards)
        cap = pkg.payload_capacity(n_bytes, shards)
        n_dev = rc[0, :1].clone()
        fin, dead = z(shards, torch.int16), z(max((shards + 63) // 64, 1), torch.int64)
        pin = z(shards * pkg.PENDING_STRIDE, torch.uint8)

        def outputs():
            return dict(srt=torch.empty(n_lines, dtype=torch.int64, device=dev),
                        pk=torch.empty(2 * mp, dtype=torch.int64, device=dev), counts=z(3, torch.int64),
                        fout=z(shards, torch.int16), pout=z(shards * pkg.PENDING_STRIDE, torch.uint8),
                        arena=torch.empty(cap, dtype=torch.uint8, device=dev),
                        offs=torch.empty(mp + 1, dtype=torch.int32, device=dev), total=z(1, torch.int64))

        a, o = outputs(), outputs()

        def direct():
            r.pack_packets(rr.data_ptr(), n_dev.data_ptr(), n_lines, fin.data_ptr(), None, a["srt"].data_ptr(),
                           a["pk"].data_ptr(), mp, a["counts"].data_ptr(), a["fout"].data_ptr())
            r.pack_payloads((rb.data_ptr(), n_bytes, a["srt"].data_ptr(), n_lines, a["pk"].data_ptr(), mp,
                             a["counts"].data_ptr(), a["fout"].data_ptr(), pin.data_ptr(), a["pout"].data_ptr(),
                             a["arena"].data_ptr(), cap, a["offs"].data_ptr(), a["total"].data_ptr()))

        ob = pkg.SrOwnerBatch(
            d_recv_bytes=rb.data_ptr(), recv_nbytes=n_bytes, d_recv_recs=rr.data_ptr(), max_records=n_lines,
            d_recv_counts=rc.data_ptr(), world=1, d_all_dead=dead.data_ptr(), d_fill_in=fin.data_ptr(),
            d_sorted=o["srt"].data_ptr(), d_packets=o["pk"].data_ptr(), max_packets=mp,
            d_counts=o["counts"].data_ptr(), d_fill_out=o["fout"].data_ptr(), d_pend_in=pin.data_ptr(),
            d_pend_out=o["pout"].data_ptr(), d_payload=o["arena"].data_ptr(), payload_cap=cap,
            d_offsets=o["offs"].data_ptr(), d_total=o["total"].data_ptr())
        owner = lambda: r.owner_pack(ob)
        direct()
        owner()
        stream.synchronize()
        n_packets, total = int(a["counts"][0].item()), int(a["total"].item())
        same = (torch.equal(a["counts"], o["counts"]) and torch.equal(a["srt"], o["srt"])
                and torch.equal(a["pk"][: 2 * n_packets], o["pk"][: 2 * n_packets])
                and torch.equal(a["offs"][: n_packets + 1], o["offs"][: n_packets + 1])
                and torch.equal(a["arena"][:total], o["arena"][:total]) and torch.equal(a["fout"], o["fout"])
                and torch.equal(a["total"], o["total"]))
        if not same or n_packets > mp or total > cap:
            raise SystemExit("sr_owner_pack and the direct calls differ on the same receive buffer")
        # the flush: 64 full slots
        fill0 = torch.full((shards,), 1450, dtype=torch.int16, device=dev)
        ffill = fill0.clone()
        fpk, fcounts = torch.empty(2 * shards, dtype=torch.int64, device=dev), z(3, torch.int64)
        fcap = pkg.payload_capacity(0, shards)
        farena, foffs, ftotal = z(fcap, torch.uint8), z(shards + 1, torch.int32), z(1, torch.int64)

        def flush():
            ffill.copy_(fill0)
            r.flush_pending(ffill.data_ptr(), pin.data_ptr(), fpk.data_ptr(), shards, fcounts.data_ptr(),
                            farena.data_ptr(), fcap, foffs.data_ptr(), ftotal.data_ptr())

        flush()
        stream.synchronize()
        if int(ftotal.item()) != 1450 * shards or int(ffill.abs().sum().item()) != 0:
            raise SystemExit("sr_flush_pending did not flush 64 full slots")
        graphs = {}
        for name, fn in (("direct", direct), ("owner", owner), ("flush", flush)):
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name], stream=stream):
                fn()
        for g in graphs.values():   # warm-up
            timed(g.replay, 3, torch)
        ms = {k: [] for k in graphs}
        for _ in range(rounds):
            for k, g in graphs.items():
                ms[k].append(timed(g.replay, reps if k != "flush" else 10 * reps, torch))
        stream.synchronize()
    return {
        "config": cfg, "desc": desc, "batches": M, "shards": shards, "world": 1, "recv_bytes": n_bytes,
        "recv_lines": n_lines, "packets": n_packets, "arena_bytes": total, "reps": reps, "rounds": rounds,
        "direct_ms": ms["direct"], "owner_pack_ms": ms["owner"], "flush_64_ms": ms["flush"],
        "owner_minus_direct_us": [1e3 * (x - y) for x, y in zip(ms["owner"], ms["direct"])],
        "outputs_identical": True,
        "timing": "device events around back-to-back graph replays, one captured graph per leg, rounds alternate "
                  "the legs; flush includes the 128-byte copy that refills the fills",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("owner_pack_bench needs a GPU: nothing is measured without one")
    pkg = importlib.import_module("statsd-router_amd")
    line = run(pkg, torch, args.config, args.reps, args.rounds)
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
