"""GPU: the in-process communicator (sr_comm_group_open / sr_comm_open_local). Ranks are threads of the
test process on one GPU, each with its own context and stream; every comm has a 60 s deadline and the
threads are joined with a limit, so a failure never hangs. The C calls the multi-GPU run makes
(sr_regroup_launch, sr_exchange_sizes with peers, sr_exchange_data, sr_exchange_dead, sr_owner_pack) run
here with 2, 3 and 8 ranks, against the oracle; every output is poisoned and compared whole."""
from __future__ import annotations

import errno
import importlib
import time

import numpy as np
import pytest

import local_comm_ranks as R
import owner_expect as O
import payload_expect as X
from test_gpu_regroup import _expected_receive, _rank_inputs

pytestmark = pytest.mark.gpu

GUARD = 64


# ---- 1. the pull kernel, every edge ------------------------------------------------------------------
def _edge_segments():
    """(length, source misalignment, destination misalignment): the 16-byte unit's edges on both sides."""
    return [(n, s, d) for n in (1, 15, 16, 17, 4097) for s in (0, 1, 4, 15) for d in (0, 3, 8, 15)]


PULL_CASES = {
    "edges": _edge_segments(),
    "one_large": [((1 << 20) + 5, 5, 11)],                                      # many 16 KiB pieces
    "200_small": [(1 + (37 * i) % 301, (7 * i) % 16, (5 * i) % 16) for i in range(200)],   # > 192: two launches
}


def _layout(segs):
    """Byte offsets of every segment in a 16-byte aligned source arena and in a destination arena where
    each destination sits between GUARD bytes: (src offsets, dst offsets, src size, dst size)."""
    so, do, s_at, d_at = [], [], 0, 0
    for n, smis, dmis in segs:
        so.append(s_at + smis)
        s_at += (smis + n + 31) // 16 * 16
        do.append(d_at + GUARD + dmis)
        d_at += (GUARD + dmis + n + GUARD + 15) // 16 * 16
    return so, do, s_at, d_at


@pytest.mark.parametrize("case", list(PULL_CASES))
def test_pull_kernel_every_edge(pkg, case):
    """World 2, both directions in one group through CommTransport: every receive arena equals the peer's
    source bytes at the destinations and 0xCD everywhere else (the guards around every destination)."""
    import torch

    segs = PULL_CASES[case]
    so, do, s_size, d_size = _layout(segs)
    sources = [np.random.default_rng(4100 + r).integers(0, 256, s_size, dtype=np.uint8) for r in range(2)]
    ranks = R.LocalRanks(pkg, 2)

    def rank_main(r):
        peer = 1 - r
        src = torch.from_numpy(sources[r]).to("cuda")
        dst = torch.full((d_size,), 0xCD, dtype=torch.uint8, device="cuda")
        assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        with pkg.Router(4, 1 << 16) as router, ranks.comm(r) as comm:
            t = pkg.CommTransport(comm, router)
            t.group_start()
            for i, (n, _, _) in enumerate(segs):
                t.send(src.data_ptr() + so[i], n, peer, i % 3)
                t.recv(dst.data_ptr() + do[i], n, peer, i % 3)
            t.group_end()
            router.sync()
            return dst.cpu().numpy()

    try:
        got = R.run_threads(2, rank_main)
    finally:
        ranks.close()
    for r in range(2):
        want = np.full(d_size, 0xCD, dtype=np.uint8)
        for i, (n, _, _) in enumerate(segs):
            want[do[i]: do[i] + n] = sources[1 - r][so[i]: so[i] + n]
        bad = np.nonzero(got[r] != want)[0]
        assert bad.size == 0, (case, r, bad[:8].tolist())


# ---- 2. sr_regroup_launch on local comms -------------------------------------------------------------
@pytest.mark.parametrize("world,n_shards", [(2, 64), (3, 16), (8, 64), (3, 1)])
def test_regroup_launch_local_ranks(pkg, oracle, world, n_shards):
    """test_regroup_run_device_ranks' inputs and checks on sr_regroup_launch over in-process comms: the
    shipped sequence (sizes all-to-all with a real `recv` in sizes_publish_kernel, plan, scatter with the
    own chunk in place, grouped sends and receives, rebase) with `world` ranks. Two launches per rank; the
    last rank's first launch is one record short (-ENOSPC) and finishes with sr_pack_owner_scatter (own -1)
    + sr_exchange_data while its peers wait inside their call."""
    import torch

    inputs = [_rank_inputs(pkg, oracle, r, world, n_shards) for r in range(world)]
    ranks = R.LocalRanks(pkg, world)

    def rank_main(r):
        datas, _, alive = inputs[r]
        nb = len(datas)
        cap = max(d.size for d in datas)
        d_in = torch.zeros((nb, cap), dtype=torch.uint8, device="cuda")
        for b, d in enumerate(datas):
            d_in[b, : d.size].copy_(torch.from_numpy(d.copy()))
        d_rec = torch.zeros((nb, cap), dtype=torch.int64, device="cuda")
        d_n = torch.zeros(nb, dtype=torch.int64, device="cuda")
        pcap = pkg.pack_capacity(sum(int(d.size) for d in datas))
        packed = torch.zeros(pcap, dtype=torch.uint8, device="cuda")
        precs = torch.zeros(nb * cap, dtype=torch.int64, device="cuda")
        counts = torch.zeros((world, 2), dtype=torch.int64, device="cuda")
        eb, er, ec = _expected_receive(oracle, inputs, world, r)
        got = []
        with pkg.Router(n_shards, cap) as router, ranks.comm(r) as comm:
            router.set_alive(alive)
            batches = [(d_in[b].data_ptr(), int(d.size), d_rec[b].data_ptr(), cap, d_n[b].data_ptr())
                       for b, d in enumerate(datas)]
            torch.cuda.synchronize()
            router.route_device_many([(db, n, dr, mr, None, dn) for db, n, dr, mr, dn in batches])
            for step in range(2):
                short = step == 0 and r == world - 1 and len(er) > 0
                nl = max(len(er) - (1 if short else 0), 1)
                rb = torch.full((eb.size + 64,), 0xCD, dtype=torch.uint8, device="cuda")
                rr = torch.full((nl,), -1, dtype=torch.int64, device="cuda")
                rcv = torch.full((world, 2), -1, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                fits, sent, received = router.regroup_launch(
                    comm, batches, counts.data_ptr(), rcv.data_ptr(), packed.data_ptr(), pcap, precs.data_ptr(),
                    rb.data_ptr(), rb.numel(), rr.data_ptr(), nl)
                assert fits == (not short), (r, step, fits)
                if not fits:
                    rr = torch.full((len(er),), -1, dtype=torch.int64, device="cuda")
                    torch.cuda.synchronize()
                    router.pack_owner_scatter(batches, world, -1, 0, 0, packed.data_ptr(), pcap, precs.data_ptr())
                    router.exchange_data(comm, packed.data_ptr(), precs.data_ptr(), sent, received, rb.data_ptr(),
                                         rr.data_ptr())
                router.sync()
                got.append((rb.cpu().numpy(), rr.cpu().numpy().view(pkg.RECORD_DTYPE)[: len(er)],
                            received.astype(np.int64), rcv.cpu().numpy()))
        return got, eb, er, ec

    try:
        out = R.run_threads(world, rank_main, limit=240)
    finally:
        ranks.close()
    assert any(len(out[r][2]) for r in range(world))   # some rank received lines
    for r in range(world):
        got, eb, er, ec = out[r]
        for step, (rb, rr, received, rcv) in enumerate(got):
            assert received.tolist() == ec.tolist() == rcv.tolist(), (r, step)
            assert np.array_equal(rb[: eb.size], eb), (r, step)
            assert (rb[eb.size:] == 0xCD).all(), (r, step)
            assert np.array_equal(rr, er), (r, step)


# ---- 3. the owner path -------------------------------------------------------------------------------
def _state(n, seed):
    rng = np.random.default_rng(seed)
    fills = rng.choice([0, 1, 700, 1449, 1450], n).astype(np.int64)
    some = rng.random(n) < 0.5
    fills[some] = rng.integers(0, 1451, int(some.sum()))
    return fills.tolist(), X.random_pending(rng, fills)


@pytest.mark.parametrize("world,n", [(2, 16), (3, 64)])
def test_owner_path_on_local_comms(pkg, oracle, world, n):
    """sr_regroup_launch -> sr_exchange_dead(comm) -> sr_owner_pack, two launches chained on the device,
    against OwnerExpect."""
    launches = [[O.rank_inputs(pkg, oracle, r, world, n, seed=2300 + 10 * world + n + 50 * step)
                 for r in range(world)] for step in range(2)]
    states = [_state(n, 41 * world + n + r) for r in range(world)]
    fills, pend = [s[0] for s in states], [s[1] for s in states]
    ck = R.OwnerChecker(pkg, oracle, n, launches, fills, pend)
    R.run_owner_ranks(pkg, n, launches, fills, pend, ck)
    assert len(ck.expect) == 2 * world
    assert any(e.n_lines > 0 and len(e.packets) > 0 for e in ck.expect.values())
    assert any(e.dead for e in ck.expect.values())


def test_owner_path_differing_snapshots(pkg, oracle):
    """Rank 0 routes with shard k dead (and probes it), rank 1 the same bytes with k alive: k's owner drops
    k's old pending bytes first and keeps rank 1's lines (carry 0). Two launches chained."""
    world, n = 2, 4
    launches = []
    for step in range(2):
        datas = [O.batch_bytes(pkg, 2900 + 10 * step + b, 4096 + 1000 * b) for b in range(2)]
        all_alive = oracle.route(datas[0], n)[0]
        k = int(all_alive["route"][all_alive["route"] < n][0])
        launches.append([(datas, [oracle.route(d, n, alive)[0] for d in datas], alive)
                         for alive in ([int(s != k) for s in range(n)], [1] * n)])
        if step == 0:
            k0 = k
    fills = [[700] * n for _ in range(world)]
    pend = [X.random_pending(np.random.default_rng(15 + r), fills[r]) for r in range(world)]
    ck = R.OwnerChecker(pkg, oracle, n, launches, fills, pend)
    R.run_owner_ranks(pkg, n, launches, fills, pend, ck)
    assert k0 in O.source_dead(oracle, launches[0][0], n) and k0 not in O.source_dead(oracle, launches[0][1], n)
    e = ck.expect[(k0 % world, 0)]
    mine = e.packets[e.packets["shard"] == k0]
    assert len(mine) and int(mine[0]["carry"]) == 0 and int(e.fill_out[k0]) > 0


# ---- 4. two communicators alternating ----------------------------------------------------------------
def test_two_communicators_alternate(pkg, oracle):
    """World 2, two groups: each rank drives two LaunchRegrouper(comm=...) on two contexts and streams, taking
    alternate steps (three each, the same order on both ranks), nothing synchronised in between."""
    import torch

    rg = importlib.import_module("statsd-router_amd.regroup")
    world, n, steps = 2, 16, 3
    inputs = {(k, s): [O.rank_inputs(pkg, oracle, r, world, n, seed=3100 + 100 * k + 10 * s) for r in range(world)]
              for k in range(2) for s in range(steps)}
    groups = [R.LocalRanks(pkg, world), R.LocalRanks(pkg, world)]

    def rank_main(r):
        cap = max(d.size for inp in inputs.values() for d in inp[r][0])
        total = max(sum(int(d.size) for d in inp[r][0]) for inp in inputs.values())
        keep, results = [], {}
        with pkg.Router(n, cap) as r0, pkg.Router(n, cap) as r1, groups[0].comm(r) as c0, groups[1].comm(r) as c1:
            routers, comms = (r0, r1), (c0, c1)
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            regs = []
            for k in range(2):
                routers[k].set_stream(streams[k].cuda_stream)
                regs.append(rg.LaunchRegrouper(pkg, routers[k], total, 2 * cap, comm=comms[k]))
            # every step's inputs resident before the first launch
            for (k, s), inp in inputs.items():
                datas, _, alive = inp[r]
                d_in = torch.zeros((len(datas), cap), dtype=torch.uint8, device="cuda")
                for b, d in enumerate(datas):
                    d_in[b, : d.size].copy_(torch.from_numpy(d.copy()))
                d_rec = torch.zeros((len(datas), cap), dtype=torch.int64, device="cuda")
                d_n = torch.zeros(len(datas), dtype=torch.int64, device="cuda")
                keep.append((k, s, alive, d_in, d_rec, d_n, [int(d.size) for d in datas]))
            torch.cuda.synchronize()
            for s in range(steps):
                for k in range(2):
                    _, _, alive, d_in, d_rec, d_n, sizes = next(x for x in keep if x[0] == k and x[1] == s)
                    routers[k].set_alive(alive)
                    batches = [(d_in[b].data_ptr(), sizes[b], d_rec[b].data_ptr(), cap, d_n[b].data_ptr())
                               for b in range(len(sizes))]
                    routers[k].route_device_many([(db, nb, dr, mr, None, dn) for db, nb, dr, mr, dn in batches])
                    results[(k, s)] = regs[k](batches) + (regs[k].last_received,)
            for st in streams:
                st.synchronize()
            return {key: (rb.cpu().numpy(), rr.cpu().numpy().view(pkg.RECORD_DTYPE), rc.cpu().numpy().tolist(), lr)
                    for key, (rb, rr, rc, lr) in results.items()}

    try:
        out = R.run_threads(world, rank_main)
    finally:
        for g in groups:
            g.close()
    for r in range(world):
        for key, (rb, rr, rc, last_received) in out[r].items():
            eb, er, ec = O.expected_receive(oracle, inputs[key], world, r)
            assert rc == ec.tolist() == last_received, (r, key)
            assert np.array_equal(rb, eb), (r, key)
            assert np.array_equal(rr, er), (r, key)


# ---- 5. an absent peer -------------------------------------------------------------------------------
def test_absent_peer_times_out(pkg):
    """Rank 0 alone calls sr_exchange_sizes with a 200 ms deadline: -ETIMEDOUT (the wall-clock cap only
    guards against a wait that ignores the deadline), nothing left enqueued (sr_sync returns), then -EPIPE
    at once for the latecomer; both comms and the group close. By the invariant nothing on the device
    waits, so this provokes no stall."""
    import torch

    g = pkg.CommGroup(2)
    d_cnt = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    d_rcv = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    c0 = pkg.Comm.local(g, 0, 0)
    c0.set_timeout(200)
    with pkg.Router(4, 1 << 16) as r0, pkg.Router(4, 1 << 16) as r1:
        t0 = time.monotonic()
        with pytest.raises(pkg.SrError) as e:
            r0.exchange_sizes(c0, d_cnt.data_ptr(), d_rcv.data_ptr())
        waited = time.monotonic() - t0
        assert e.value.errno == errno.ETIMEDOUT
        assert 0.2 <= waited < 5.0, waited
        r0.sync()
        with pytest.raises(pkg.SrError) as e:   # the comm is broken for its own rank too
            r0.exchange_sizes(c0, d_cnt.data_ptr(), d_rcv.data_ptr())
        assert e.value.errno == errno.EPIPE
        c1 = pkg.Comm.local(g, 1, 0)
        c1.set_timeout(R.TIMEOUT_MS)
        t0 = time.monotonic()
        with pytest.raises(pkg.SrError) as e:
            r1.exchange_sizes(c1, d_cnt.data_ptr(), d_rcv.data_ptr())
        assert e.value.errno == errno.EPIPE and time.monotonic() - t0 < 1.0
        r1.sync()
        c0.close()
        c1.close()
    g.close()
    assert not g.handle


# ---- 6. errors ---------------------------------------------------------------------------------------
def test_size_mismatch_breaks_the_group(pkg):
    """A receive of 8 bytes against a send of 16: -EMSGSIZE at the receiver, nothing copied, the group
    broken for both ranks."""
    import torch

    ranks = R.LocalRanks(pkg, 2)

    def rank_main(r):
        buf = torch.full((64,), 0x11 if r == 0 else 0xCD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with pkg.Router(4, 1 << 16) as router, ranks.comm(r) as comm:
            t = pkg.CommTransport(comm, router)
            t.group_start()
            if r == 0:
                t.send(buf.data_ptr(), 16, 1, 1)
            else:
                t.recv(buf.data_ptr() + 16, 8, 0, 1)
            with pytest.raises(pkg.SrError) as e:
                t.group_end()
            first = e.value.errno
            with pytest.raises(pkg.SrError) as e:
                t.group_start()
            router.sync()
            return first, e.value.errno, buf.cpu().numpy()

    try:
        out = R.run_threads(2, rank_main)
    finally:
        ranks.close()
    assert out[1][0] == errno.EMSGSIZE and out[0][0] == errno.EPIPE
    assert out[0][1] == errno.EPIPE and out[1][1] == errno.EPIPE
    assert (out[1][2] == 0xCD).all() and (out[0][2] == 0x11).all()


def test_rank_taken_and_group_busy(pkg):
    """A rank opened twice is -EBUSY; the group does not close while a comm of it is open; a send outside
    a group or to the rank itself is -EINVAL."""
    g = pkg.CommGroup(2)
    c = pkg.Comm.local(g, 0, 0)
    try:
        with pytest.raises(pkg.SrError) as e:
            pkg.Comm.local(g, 0, 0)
        assert e.value.errno == errno.EBUSY
        with pytest.raises(pkg.SrError) as e:
            g.close()
        assert e.value.errno == errno.EBUSY and g.handle
        with pkg.Router(4, 1 << 16) as router:
            t = pkg.CommTransport(c, router)
            with pytest.raises(pkg.SrError) as e:
                t.send(4096, 8, 1, 0)   # no group open
            assert e.value.errno == errno.EINVAL
            t.group_start()
            with pytest.raises(pkg.SrError) as e:
                t.send(4096, 8, 0, 0)   # to itself
            assert e.value.errno == errno.EINVAL
            t.group_end()               # nothing posted: returns at once, no peer needed
            router.sync()
    finally:
        c.close()
    c2 = pkg.Comm.local(g, 0, 0)   # the rank is free again
    c2.close()
    g.close()
