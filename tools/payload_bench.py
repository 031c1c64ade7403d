#!/usr/bin/env python3
"""sr_pack_payloads_many alone, against a plain device copy of the same bytes and the owner scatter.

The resident inputs and launch shape of bench.py's route_pack leg: 32 batches of 16 MiB per launch,
configs C2-C5, every shard alive. Per config, one eager sr_route_pack_many writes the descriptors; then,
in one process, three rounds alternate
  payload : sr_pack_payloads_many over the 32 batches (pending buffers on the device), one captured graph;
  copy    : torch's device copy of as many bytes as the arena holds (tools/copy_bw.py's measure);
  owner   : sr_pack_many_by_owner with one owner over the same batches, one captured graph,
each timed with events around back-to-back runs after a warm-up. The gather reads and writes every byte
once, like the copy, which is the yardstick. One JSON line per config on stdout and, with --out, in a
file; --remarks adds the payload kernels' register / LDS / occupancy figures from a build's
-Rpass-analysis=kernel-resource-usage output (tools/resource_usage.py).

  python tools/payload_bench.py [--configs c2,c3,c4,c5] [--reps 50] [--out FILE] [--remarks FILE]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

import numpy as np

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


def run_config(pkg, torch, cfg, reps, rounds):
    from bench import CONFIGS

    desc, batch_bytes, lens, p_inv, shards, seed0, _ = CONFIGS[cfg]
    M = pkg.SR_MAX_BATCHES_PER_LAUNCH
    dev = torch.device("cuda", 0)
    host = [pkg.gen_stream(batch_bytes, lens, seed=seed0 + 65_537 * b, p_invalid=p_inv) for b in range(M)]
    sizes = [int(s.data.size) for s in host]
    max_lines = max(int(s.n_lines) for s in host)
    mp = pkg.max_packets(batch_bytes, shards)
    cap = pkg.payload_capacity(batch_bytes, shards)
    cap16 = (cap + 15) & ~15
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream), pkg.Router(shards, batch_bytes, device=0) as r:
        r.set_stream(stream.cuda_stream)
        d_in = torch.empty((M, batch_bytes), dtype=torch.uint8, device=dev)
        for b, s in enumerate(host):
            d_in[b, : sizes[b]].copy_(torch.from_numpy(s.data))
        rec = torch.empty((M, max_lines), dtype=torch.int64, device=dev)
        srt = torch.empty((M, max_lines), dtype=torch.int64, device=dev)
        cnt = torch.zeros(M, dtype=torch.int64, device=dev)
        pk = torch.empty((M, mp * 2), dtype=torch.int64, device=dev)
        counts = torch.zeros((M, 3), dtype=torch.int64, device=dev)
        fill = torch.zeros((M, shards), dtype=torch.int16, device=dev)
        fout = torch.zeros((M, shards), dtype=torch.int16, device=dev)
        pd = torch.zeros((M, max((shards + 63) // 64, 1)), dtype=torch.int64, device=dev)
        r.route_pack_many([(d_in[b].data_ptr(), sizes[b], rec[b].data_ptr(), max_lines, None, cnt[b].data_ptr(),
                            pd[b].data_ptr(), fill[b].data_ptr(), srt[b].data_ptr(), pk[b].data_ptr(), mp,
                            counts[b].data_ptr(), fout[b].data_ptr()) for b in range(M)])
        stream.synchronize()
        # the payloads
        arena = torch.empty((M, cap16), dtype=torch.uint8, device=dev)
        offs = torch.empty((M, mp + 1), dtype=torch.int32, device=dev)
        total = torch.zeros(M, dtype=torch.int64, device=dev)
        pin = torch.zeros((M, shards * pkg.PENDING_STRIDE), dtype=torch.uint8, device=dev)
        pout = torch.zeros((M, shards * pkg.PENDING_STRIDE), dtype=torch.uint8, device=dev)
        pb = r.payload_batches([(d_in[b].data_ptr(), sizes[b], srt[b].data_ptr(), max_lines, pk[b].data_ptr(), mp,
                                 counts[b].data_ptr(), fout[b].data_ptr(), pin[b].data_ptr(), pout[b].data_ptr(),
                                 arena[b].data_ptr(), cap, offs[b].data_ptr(), total[b].data_ptr()) for b in range(M)])
        r.pack_payloads_many(pb)
        stream.synchronize()
        n_bytes = int(total.sum().item())
        n_packets = int(counts[:, 0].sum().item())
        n_lines = int(counts[:, 1].sum().item())
        # spot check against the descriptors: the arena's first packet of batch 0 is its first lines
        first = np.frombuffer(pk[0].cpu().numpy().tobytes(), dtype=pkg.PACKET_DTYPE)[0]
        recs0 = np.frombuffer(srt[0].cpu().numpy().tobytes(), dtype=pkg.RECORD_DTYPE)
        want = b"".join(host[0].data[int(q["offset"]): int(q["offset"]) + int(q["length"])].tobytes()
                        for q in recs0[int(first["first"]): int(first["first"]) + int(first["nlines"])])
        got = arena[0, : len(want)].cpu().numpy().tobytes()
        if got != want:
            raise SystemExit(f"{cfg}: the arena's first packet differs from its lines")
        g_pay = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_pay, stream=stream):
            r.pack_payloads_many(pb)
        # the copy: as many bytes as the arena holds
        a = torch.randint(0, 255, (n_bytes,), dtype=torch.uint8, device=dev)
        c = torch.empty_like(a)
        # the owner scatter, one owner
        ob = [(d_in[b].data_ptr(), sizes[b], rec[b].data_ptr(), max_lines, cnt[b].data_ptr()) for b in range(M)]
        ocap = pkg.pack_capacity(sum(sizes))
        o_bytes = torch.empty(ocap, dtype=torch.uint8, device=dev)
        o_recs = torch.empty(M * max_lines, dtype=torch.int64, device=dev)
        o_counts = torch.zeros(2, dtype=torch.int64, device=dev)
        r.pack_many_by_owner(ob, 1, o_bytes.data_ptr(), ocap, o_recs.data_ptr(), o_counts.data_ptr())
        stream.synchronize()
        g_own = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_own, stream=stream):
            r.pack_many_by_owner(ob, 1, o_bytes.data_ptr(), ocap, o_recs.data_ptr(), o_counts.data_ptr())
        legs = {"payload": g_pay.replay, "copy": lambda: c.copy_(a), "owner": g_own.replay}
        for fn in legs.values():   # warm-up
            timed(fn, 5, torch)
        ms = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                ms[k].append(timed(fn, reps, torch))
        stream.synchronize()
    best = {k: min(v) for k, v in ms.items()}
    return {
        "config": cfg, "desc": desc, "batches": M, "batch_bytes": batch_bytes, "shards": shards,
        "arena_bytes": n_bytes, "packets": n_packets, "valid_lines": n_lines, "reps": reps, "rounds": rounds,
        "payload_ms": ms["payload"], "copy_ms": ms["copy"], "owner_scatter_ms": ms["owner"],
        "payload_over_copy": best["payload"] / best["copy"], "owner_over_copy": best["owner"] / best["copy"],
        "payload_TBps_rw": 2 * n_bytes / best["payload"] / 1e9, "copy_TBps_rw": 2 * n_bytes / best["copy"] / 1e9,
        "timing": "device events around back-to-back runs, best of the rounds for the ratios; payload and owner "
                  "scatter each one captured graph per run, the copy torch's Tensor.copy_",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3,c4,c5")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--remarks", help="stderr of a build with -Rpass-analysis=kernel-resource-usage")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("payload_bench needs a GPU: nothing is measured without one")
    pkg = importlib.import_module("statsd-router_amd")
    lines = []
    if args.remarks:
        import resource_usage

        res = {k: v for k, v in resource_usage.parse(args.remarks).items() if "payload" in k}
        lines.append({"kernel_resources": dict(zip(resource_usage.demangle(sorted(res)), [res[k] for k in sorted(res)]))})
    for cfg in args.configs.split(","):
        lines.append(run_config(pkg, torch, cfg, args.reps, args.rounds))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
