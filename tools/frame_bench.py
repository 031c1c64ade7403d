"""Device framing, measured. One JSON line per measurement on stdout.

  device : sr_frame_slots on device-resident slots against a plain device copy of the same number of framed
           bytes (tools/copy_bw.py's way: torch copy_, device events), for a 16 MiB framed batch of ~1.4 KB
           datagrams of 64-byte lines (C1's shape) and of 64-byte single-line datagrams (more than
           SR_MAX_SLOTS of them: several calls, timed together);
  host   : per batch, wall time and the calling thread's CPU time of
             framed : sr_frame_datagrams into a page-locked batch + sr_route_pack_submit (the host-framing path)
             slots  : sr_route_pack_submit_slots on the same datagrams in their page-locked slots
           slots 0 and 1 alternating, every batch ending with sr_route_pack_result.
Variants alternate within a round; --rounds rounds. The C1 loopback A/B is tools/loopback/c1_bench.py with
--var framing:SR_DEVICE_FRAMING=1.

    python tools/frame_bench.py [--rounds 3] [--iters 30] [--device-iters 2000] [--mib 16]
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("statsd-router_amd")

STRIDE = 4096


def datagrams(shape: str, nbytes: int):
    """(arena uint8 [count * STRIDE], lens uint16, framed bytes): datagrams of 64-byte lines, 22 lines
    (1408 bytes) each for "c1", one line each for "single"; every datagram ends in '\\n'."""
    per = 1408 if shape == "c1" else 64
    count = nbytes // per
    s = pkg.gen_stream(count * per, [64], seed=0xF7A3E)
    assert s.data.size == count * per
    arena = np.zeros((count, STRIDE), dtype=np.uint8)
    arena[:, :per] = s.data.reshape(count, per)
    return arena.reshape(-1), np.full(count, per, dtype=np.uint16), s.data


def bench_device(shape: str, nbytes: int, rounds: int, iters: int):
    import torch

    arena, lens, framed = datagrams(shape, nbytes)
    count, total = int(lens.size), int(framed.size)
    d_arena = torch.from_numpy(arena).cuda()
    d_lens = torch.from_numpy(lens.view(np.int16)).cuda()
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_src = torch.from_numpy(framed.copy()).cuda()
    d_cpy = torch.empty_like(d_src)
    d_total = torch.zeros(8, dtype=torch.int64, device="cuda")
    calls = [(j0, min(pkg.SR_MAX_SLOTS, count - j0)) for j0 in range(0, count, pkg.SR_MAX_SLOTS)]
    per = int(lens[0])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), pkg.Router(4, 1 << 16) as r:
        r.set_stream(stream.cuda_stream)

        def frame():
            for k, (j0, n) in enumerate(calls):
                r.frame_slots(d_arena.data_ptr() + j0 * STRIDE, STRIDE, d_lens.data_ptr() + 2 * j0, n,
                              d_out.data_ptr() + j0 * per, total - j0 * per, None, d_total.data_ptr() + 8 * k)

        def copy():
            d_cpy.copy_(d_src)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / iters

        for _ in range(5):
            frame()
            copy()
        torch.cuda.synchronize()
        assert torch.equal(d_out, d_src), "framed batch differs from the datagrams' bytes"
        for rnd in range(rounds):
            f_ms, c_ms = timed(frame), timed(copy)
            print(json.dumps({"what": "device", "shape": shape, "round": rnd, "datagrams": count, "framed_bytes": total,
                              "calls": len(calls), "frame_ms": round(f_ms, 4), "copy_ms": round(c_ms, 4),
                              "frame_GBps_rw": round(2 * total / f_ms / 1e6, 1),
                              "copy_GBps_rw": round(2 * total / c_ms / 1e6, 1),
                              "frame_over_copy": round(f_ms / c_ms, 2)}), flush=True)


def bench_host(n_slots: int, rounds: int, iters: int):
    arena_np, lens, framed = datagrams("c1", n_slots * 1408)
    count, total = int(lens.size), int(framed.size)
    L = pkg.lib()
    arenas = [pkg.HostBuffer(arena_np.size) for _ in range(2)]
    batches = [pkg.HostBuffer(total + 1) for _ in range(2)]   # sr_frame_datagrams wants room for one more '\n'
    for a in arenas:
        a.array[:] = arena_np
    ptrs = [(ctypes.c_void_p * count)(*[a.addr + j * STRIDE for j in range(count)]) for a in arenas]
    lens_sz = (ctypes.c_size_t * count)(*[int(x) for x in lens])
    lens16 = np.ascontiguousarray(lens)
    res = pkg.SrPackResult()
    with pkg.Router(16, total) as ra, pkg.Router(16, total) as rb:

        def framed_batch(i):
            k = i & 1
            n = L.sr_frame_datagrams(ctypes.c_void_p(batches[k].addr), total + 1, ptrs[k], lens_sz, count)
            assert n == total
            rc = L.sr_route_pack_submit(ra.handle, k, ctypes.c_void_p(batches[k].addr), n, None)
            rc = rc or L.sr_route_pack_result(ra.handle, k, ctypes.byref(res))
            assert rc == 0, rc
            return res.n_records

        def slots_batch(i):
            k = i & 1
            rc = L.sr_route_pack_submit_slots(rb.handle, k, ctypes.c_void_p(arenas[k].addr), STRIDE, lens16.ctypes.data,
                                              count, None)
            rc = rc or L.sr_route_pack_result(rb.handle, k, ctypes.byref(res))
            assert rc == 0, rc
            return res.n_records

        def timed(fn):
            w0, c0 = time.perf_counter(), time.thread_time()
            for i in range(iters):
                fn(i)
            return (time.perf_counter() - w0) / iters * 1e3, (time.thread_time() - c0) / iters * 1e3

        for i in range(6):
            assert framed_batch(i) == slots_batch(i) == total // 64
        for rnd in range(rounds):
            for name, fn in (("framed", framed_batch), ("slots", slots_batch)):
                wall, cpu = timed(fn)
                print(json.dumps({"what": "host", "variant": name, "round": rnd, "datagrams": count,
                                  "framed_bytes": total, "wall_ms_per_batch": round(wall, 4),
                                  "thread_cpu_ms_per_batch": round(cpu, 4)}), flush=True)
    for b in arenas + batches:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30, help="host-path batches per timed window")
    ap.add_argument("--device-iters", type=int, default=2000, help="device calls per timed window")
    ap.add_argument("--mib", type=int, default=16, help="framed MiB of a device batch")
    ap.add_argument("--host-slots", type=int, default=2048, help="datagrams of a host-path batch (8 MiB of slots)")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("frame_bench needs a GPU: nothing is measured without one")
    for shape in ("c1", "single"):
        bench_device(shape, a.mib << 20, a.rounds, a.device_iters)
    bench_host(a.host_slots, a.rounds, a.iters)


if __name__ == "__main__":
    main()
