"""Helpers of tests/test_gpu_local_comm.py: ranks of an in-process communicator as threads of the test
process on one GPU, and the owner-side runner and checker of tests/owner_expect.py / test_gpu_owner_pack.py
restated for communicators (sr_regroup_launch + sr_exchange_dead on pkg.Comm.local instead of the mailbox).
A plain helper module: no fixtures, no tests."""
from __future__ import annotations

import importlib
import threading
import traceback

import numpy as np

import owner_expect as O
import payload_expect as X

TIMEOUT_MS = 60000   # every comm of the tests: a failed peer costs a minute at most, never a hang


def run_threads(world, fn, limit=150):
    """fn(rank) on `world` threads, joined with a limit; a rank's exception fails the test with its
    traceback. Returns {rank: fn's result}."""
    out, errs = {}, {}

    def main(r):
        try:
            import torch

            torch.cuda.set_device(0)
            out[r] = fn(r)
        except Exception:   # noqa: BLE001
            errs[r] = traceback.format_exc()

    th = [threading.Thread(target=main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(limit)
    assert not any(t.is_alive() for t in th), "a rank did not finish"
    assert not errs, "\n".join(f"rank {r}:\n{e}" for r, e in errs.items())
    return out


class LocalRanks:
    """A group and, per rank thread, its communicator: `with ranks.comm(r) as comm:` opens rank r with the
    tests' deadline and closes it; close() closes the group (after the threads)."""

    def __init__(self, pkg, world):
        self.pkg, self.world, self.group = pkg, world, pkg.CommGroup(world)

    def comm(self, rank, timeout_ms=TIMEOUT_MS):
        ranks = self

        class _Ctx:
            def __enter__(self):
                self.c = ranks.pkg.Comm.local(ranks.group, rank, 0)
                self.c.set_timeout(timeout_ms)
                return self.c

            def __exit__(self, *exc):
                self.c.close()

        return _Ctx()

    def close(self):
        self.group.close()


class OwnerChecker:
    """The oracle's expectation per rank and launch, chained over the launches (test_gpu_owner_pack.py's
    checker): receive buffers, rebased records, received sizes, the probed-dead rows and every output of
    sr_owner_pack, compared whole."""

    def __init__(self, pkg, oracle, n, launches, fills, pendings):
        self.pkg, self.oracle, self.n, self.launches = pkg, oracle, n, launches
        self.world = len(launches[0])
        self.fills = {r: list(fills[r]) for r in range(self.world)}
        self.pend = {r: dict(pendings[r]) for r in range(self.world)}
        self.expect = {}

    def __call__(self, r, step, op, received, rb, rr, rcv):
        inputs = self.launches[step]
        eb, er, ec = O.expected_receive(self.oracle, inputs, self.world, r)
        dead = set().union(*[O.source_dead(self.oracle, inp, self.n) for inp in inputs])
        e = O.OwnerExpect(self.oracle, self.n, eb, er, dead, self.fills[r], self.pend[r])
        label = f"rank {r} launch {step}"
        assert received.astype(np.int64).tolist() == ec.tolist() == rcv.cpu().numpy().tolist(), label
        got_b = rb.cpu().numpy()
        assert np.array_equal(got_b[: eb.size], eb) and (got_b[eb.size:] == 0xCD).all(), label
        assert np.array_equal(rr.cpu().numpy().view(self.pkg.RECORD_DTYPE)[: len(er)], er), label
        rows = op.all_dead.cpu().numpy().view(np.uint64).reshape(self.world, -1)
        assert np.array_equal(rows, O.dead_rows(self.oracle, inputs, self.n)), (label, rows)
        O.check_owner(self.pkg, op, e, label)
        self.expect[(r, step)] = e
        self.fills[r], self.pend[r] = [int(f) for f in e.fill_out], dict(e.new_pending)


def run_owner_ranks(pkg, n, launches, fills, pendings, check):
    """owner_expect.run_ranks on in-process communicators: per launch and rank, route with bitmaps,
    sr_regroup_launch, sr_exchange_dead on the comm, sr_owner_pack through an OwnerPacker with poisoned
    outputs, then check(rank, step, op, received, rb, rr, d_recv_counts) after the rank's stream drained."""
    import torch

    rg = importlib.import_module("statsd-router_amd.regroup")
    world = len(launches[0])
    ranks = LocalRanks(pkg, world)

    def rank_main(r):
        nb = max(len(step[r][0]) for step in launches)
        cap = max(d.size for step in launches for d in step[r][0])
        total = max(sum(int(d.size) for d in step[r][0]) for step in launches)
        recv_cap = pkg.pack_capacity(max(sum(int(d.size) for inp in step for d in inp[0]) for step in launches)) + 64
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        d_in, d_rec, d_n = z((nb, cap), torch.uint8), z((nb, cap), torch.int64), z(nb, torch.int64)
        d_pd = z((nb, max((n + 63) // 64, 1)), torch.int64)
        pcap = pkg.pack_capacity(total)
        packed, precs = z(pcap, torch.uint8), z(nb * cap, torch.int64)
        counts, rcv = z((world, 2), torch.int64), z((world, 2), torch.int64)
        with pkg.Router(n, cap) as router, ranks.comm(r) as comm:
            op = rg.OwnerPacker(pkg, router, world, recv_cap, recv_cap, poison=O.POISON)
            op.set_pending(fills[r], X.pending_image(pendings[r], n, fills[r]))
            for step, per_rank in enumerate(launches):
                datas, _, alive = per_rank[r]
                for b, d in enumerate(datas):
                    d_in[b, : d.size].copy_(torch.from_numpy(d.copy()))
                rb = torch.full((recv_cap,), 0xCD, dtype=torch.uint8, device="cuda")
                rr = torch.full((recv_cap,), -1, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                router.set_alive(alive)
                batches = [(d_in[b].data_ptr(), int(d.size), d_rec[b].data_ptr(), cap, d_n[b].data_ptr(),
                            d_pd[b].data_ptr()) for b, d in enumerate(datas)]
                router.route_device_many([(db, k, dr, mr, None, dn, dp) for db, k, dr, mr, dn, dp in batches])
                fits, sent, received = router.regroup_launch(
                    comm, batches, counts.data_ptr(), rcv.data_ptr(), packed.data_ptr(), pcap, precs.data_ptr(),
                    rb.data_ptr(), rb.numel(), rr.data_ptr(), rr.numel())
                assert fits
                op.exchange_dead(comm, r, batches)
                op.pack(rb.data_ptr(), int(received[:, 1].sum()), rr.data_ptr(), rcv.data_ptr())
                router.sync()
                check(r, step, op, received, rb, rr, rcv)
            router.sync()

    try:
        run_threads(world, rank_main)
    finally:
        ranks.close()
