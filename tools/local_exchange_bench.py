#!/usr/bin/env python3
"""The in-process communicator's exchange on one MI355X: world 2 as threads of this process, each rank with
its own context and stream, over C5's 32-batch launch (32 x 16 MiB of mixed 64/256/1024-byte metrics, 64
shards), already routed and resident.

  (a) pull : local_pull_kernel alone. Rank 0 only sends its chunk for rank 1 (lines and records: two
             segments), rank 1 only receives, so one pull at a time owns the GPU. Device events on rank 1's
             stream around back-to-back groups, against torch's device copy of the same byte count on the
             same stream, three alternating rounds (tools/payload_bench.py's way). Each group's two host
             rendezvous happen while the previous pull still runs.
  (b) host : the host time of one group of two small segments each way, from group_start to group_end
             returning, both streams idle before (a barrier, then both ranks start). Through ctypes, so a
             few microseconds of interpreter are in it.
  (c) step : sr_regroup_launch per step on the local comm (wall time until the rank's stream has drained,
             both ranks starting together), and the same step through sr_regroup_run on the tests' mailbox
             transport, which stages every byte through the host: for context only.

One JSON line on stdout and, with --out, in a file.

  python tools/local_exchange_bench.py [--config c5] [--batches 32] [--reps 30] [--out FILE]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import threading
import time
import traceback

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

WORLD = 2


def timed(fn, reps, torch, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c5")
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=300)
    ap.add_argument("--step-reps", type=int, default=10)
    ap.add_argument("--mailbox-reps", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("local_exchange_bench needs a GPU: nothing is measured without one")
    from bench import CONFIGS
    import owner_expect as O

    pkg = importlib.import_module("statsd-router_amd")
    desc, batch_bytes, lens, p_inv, shards, seed0, _ = CONFIGS[args.config]
    M = args.batches
    # the two ranks' launches: different seeds per rank, as two sockets' traffic
    host = [[pkg.gen_stream(batch_bytes, lens, seed=seed0 + 65_537 * b + 7_919 * r, p_invalid=p_inv) for b in range(M)]
            for r in range(WORLD)]
    group = pkg.CommGroup(WORLD)
    Mailbox = O.mailbox_class(pkg, WORLD)
    barrier = threading.Barrier(WORLD)
    res, errs = [dict() for _ in range(WORLD)], {}

    def rank_main(r):
        try:
            torch.cuda.set_device(0)
            dev = torch.device("cuda", 0)
            peer = 1 - r
            sizes = [int(s.data.size) for s in host[r]]
            max_lines = max(int(s.n_lines) for s in host[r])
            total = sum(sizes)
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream), pkg.Router(shards, batch_bytes, device=0) as router:
                router.set_stream(stream.cuda_stream)
                comm = pkg.Comm.local(group, r, 0)
                comm.set_timeout(120000)
                d_in = torch.empty((M, batch_bytes), dtype=torch.uint8, device=dev)
                for b, s in enumerate(host[r]):
                    d_in[b, : sizes[b]].copy_(torch.from_numpy(s.data))
                rec = torch.empty((M, max_lines), dtype=torch.int64, device=dev)
                cnt = torch.zeros(M, dtype=torch.int64, device=dev)
                router.route_device_many([(d_in[b].data_ptr(), sizes[b], rec[b].data_ptr(), max_lines, None,
                                           cnt[b].data_ptr()) for b in range(M)])
                batches = router.owner_batches([(d_in[b].data_ptr(), sizes[b], rec[b].data_ptr(), max_lines,
                                                 cnt[b].data_ptr()) for b in range(M)])
                pcap = pkg.pack_capacity(total)
                packed = torch.empty(pcap, dtype=torch.uint8, device=dev)
                precs = torch.empty(M * max_lines, dtype=torch.int64, device=dev)
                counts = torch.zeros((WORLD, 2), dtype=torch.int64, device=dev)
                rcv = torch.zeros((WORLD, 2), dtype=torch.int64, device=dev)
                rcap_b, rcap_l = pkg.pack_capacity(2 * total), 2 * M * max_lines
                rb = torch.empty(rcap_b, dtype=torch.uint8, device=dev)
                rr = torch.empty(rcap_l, dtype=torch.int64, device=dev)

                def regroup():
                    rc = pkg.lib().sr_regroup_launch(
                        router.handle, comm.handle, batches, M, counts.data_ptr(), rcv.data_ptr(), packed.data_ptr(),
                        pcap, precs.data_ptr(), rb.data_ptr(), rcap_b, rr.data_ptr(), rcap_l, h_sent.ctypes.data,
                        h_recv.ctypes.data)
                    if rc:
                        raise pkg.SrError(-rc, "sr_regroup_launch")

                h_sent = np.zeros((WORLD, 2), dtype=np.uint64)
                h_recv = np.zeros((WORLD, 2), dtype=np.uint64)
                stream.synchronize()
                barrier.wait()
                # ---- (c) the whole step on the local comm ----
                regroup()   # warm-up (allocates the pack's scratch)
                router.sync()
                step_ms = []
                for _ in range(args.step_reps):
                    barrier.wait()
                    t0 = time.perf_counter()
                    regroup()
                    router.sync()
                    step_ms.append((time.perf_counter() - t0) * 1e3)
                res[r]["regroup_launch_ms"] = step_ms
                res[r]["sent"] = h_sent.astype(np.int64).tolist()
                res[r]["received"] = h_recv.astype(np.int64).tolist()
                # the packed buffers now hold the chunk for the peer: the pull's segments
                peers, _ = pkg.exchange_plan(WORLD, r, h_sent, h_recv)
                me = peers[peer]
                seg_send = [(packed.data_ptr() + int(me["send_byte0"]), int(me["send_bytes"])),
                            (precs.data_ptr() + 8 * int(me["send_line0"]), 8 * int(me["send_lines"]))]
                seg_recv = [(rb.data_ptr() + int(me["recv_byte0"]), int(me["recv_bytes"])),
                            (rr.data_ptr() + 8 * int(me["recv_line0"]), 8 * int(me["recv_lines"]))]
                t = pkg.CommTransport(comm, router)
                # ---- (a) the pull kernel alone: rank 0 sends, rank 1 receives ----
                n_pull = sum(n for _, n in (seg_send if r == 0 else seg_recv))

                def one_way():
                    t.group_start()
                    for tag, (addr, n) in enumerate(seg_send if r == 0 else seg_recv):
                        (t.send if r == 0 else t.recv)(addr, n, peer, tag)
                    t.group_end()

                a = torch.randint(0, 255, (max(n_pull, 16),), dtype=torch.uint8, device=dev)
                c = torch.empty_like(a)
                legs = {"pull": one_way, "copy": (lambda: c.copy_(a)) if r == 1 else (lambda: None)}
                ms = {k: [] for k in legs}
                barrier.wait()
                for k, fn in legs.items():   # warm-up
                    timed(fn, 5, torch, stream)
                for _ in range(args.rounds):
                    for k, fn in legs.items():
                        barrier.wait()
                        ms[k].append(timed(fn, args.reps, torch, stream))
                stream.synchronize()
                if r == 1:
                    res[r].update(pull_bytes=n_pull, pull_ms=ms["pull"], copy_ms=ms["copy"])
                # ---- (b) the host time of one small group, both ways ----
                small_s = torch.zeros(8192, dtype=torch.uint8, device=dev)
                small_r = torch.zeros(8192, dtype=torch.uint8, device=dev)
                stream.synchronize()
                host_us = []
                for i in range(args.host_reps + 20):
                    router.sync()
                    barrier.wait()
                    t0 = time.perf_counter()
                    t.group_start()
                    for tag in (0, 1):
                        t.send(small_s.data_ptr() + 4096 * tag, 4096, peer, tag)
                        t.recv(small_r.data_ptr() + 4096 * tag, 4096, peer, tag)
                    t.group_end()
                    if i >= 20:
                        host_us.append((time.perf_counter() - t0) * 1e6)
                router.sync()
                res[r]["group_host_us"] = host_us
                # ---- (c') the same step through the tests' mailbox (every byte staged through the host) ----
                mb = Mailbox(r, router)
                mail_ms = []
                for _ in range(args.mailbox_reps):
                    barrier.wait()
                    t0 = time.perf_counter()
                    fits, _, _ = router.regroup_run(mb, WORLD, r, batches, counts.data_ptr(), rcv.data_ptr(),
                                                    packed.data_ptr(), pcap, precs.data_ptr(), rb.data_ptr(), rcap_b,
                                                    rr.data_ptr(), rcap_l)
                    router.sync()
                    assert fits
                    mail_ms.append((time.perf_counter() - t0) * 1e3)
                res[r]["regroup_mailbox_ms"] = mail_ms
                comm.close()
        except Exception:   # noqa: BLE001
            errs[r] = traceback.format_exc()
            barrier.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(WORLD)]
    for x in th:
        x.start()
    for x in th:
        x.join(900)
    if errs or any(x.is_alive() for x in th):
        raise SystemExit("a rank failed:\n" + "\n".join(errs.values()))
    group.close()
    r1 = res[1]
    best_pull, best_copy = min(r1["pull_ms"]), min(r1["copy_ms"])
    us = np.array(res[0]["group_host_us"] + res[1]["group_host_us"])
    line = {
        "config": args.config, "desc": desc, "world": WORLD, "batches": M, "batch_bytes": batch_bytes,
        "shards": shards, "sent": [res[r]["sent"] for r in range(WORLD)],
        "pull_bytes": r1["pull_bytes"], "pull_segments": 2, "reps": args.reps, "rounds": args.rounds,
        "pull_ms": r1["pull_ms"], "copy_ms": r1["copy_ms"], "pull_over_copy": best_pull / best_copy,
        "pull_TBps_rw": 2 * r1["pull_bytes"] / best_pull / 1e9, "copy_TBps_rw": 2 * r1["pull_bytes"] / best_copy / 1e9,
        "group_host_us_median": float(np.median(us)), "group_host_us_p10": float(np.percentile(us, 10)),
        "group_host_us_p90": float(np.percentile(us, 90)), "host_reps": args.host_reps,
        "regroup_launch_ms": [res[r]["regroup_launch_ms"] for r in range(WORLD)],
        "regroup_launch_ms_median": float(np.median([x for r in range(WORLD) for x in res[r]["regroup_launch_ms"]])),
        "regroup_mailbox_ms": [res[r]["regroup_mailbox_ms"] for r in range(WORLD)],
        "timing": "pull and copy: device events on the receiver's stream around back-to-back runs, best of the "
                  "rounds for the ratio; host: perf_counter around group_start..group_end, streams idle; steps: "
                  "perf_counter from the call to the rank's stream drained, both ranks started by a barrier",
    }
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
