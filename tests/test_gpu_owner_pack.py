"""GPU: the owner side of the regroup. Route with probed-dead bitmaps -> sr_regroup_run (or
sr_regroup_launch) -> sr_exchange_dead(_run) -> sr_owner_pack, and sr_flush_pending, against the oracle:
the drop of every shard any source probed dead comes first, then the owner's stream is packed
(tests/owner_expect.py). Every output buffer is prefilled with poison and compared whole. Batches are
2-8 KiB of mixed line lengths (6, 64, 300, 1449) with about 10 % invalid lines, two per rank."""
from __future__ import annotations

import errno

import numpy as np
import pytest

import owner_expect as O
import payload_expect as X

pytestmark = pytest.mark.gpu


def _state(n, seed):
    """Random pending fills and bytes for every shard of one owner."""
    rng = np.random.default_rng(seed)
    fills = rng.choice([0, 1, 700, 1449, 1450], n).astype(np.int64)
    some = rng.random(n) < 0.5
    fills[some] = rng.integers(0, 1451, int(some.sum()))
    return fills.tolist(), X.random_pending(rng, fills)


class _Checker:
    """check() of owner_expect.run_ranks: the oracle's expectation per rank and launch, chained over the
    launches; what the GPU flushed is collected per shard from the GPU's own descriptors and arena."""

    def __init__(self, pkg, oracle, n, launches, fills, pendings):
        self.pkg, self.oracle, self.n, self.launches = pkg, oracle, n, launches
        self.world = len(launches[0])
        self.fills = {r: list(fills[r]) for r in range(self.world)}
        self.pend = {r: dict(pendings[r]) for r in range(self.world)}
        self.expect = {}      # (rank, step) -> OwnerExpect
        self.sent = {r: {} for r in range(self.world)}   # rank -> shard -> bytes flushed so far (GPU)

    def expectation(self, r, step):
        """(OwnerExpect, received counts) of rank r at `step` from the state the previous steps left."""
        inputs = self.launches[step]
        eb, er, ec = O.expected_receive(self.oracle, inputs, self.world, r)
        dead = set().union(*[O.source_dead(self.oracle, inp, self.n) for inp in inputs])
        return O.OwnerExpect(self.oracle, self.n, eb, er, dead, self.fills[r], self.pend[r]), eb, er, ec

    def collect(self, r, op):
        nd = min(int(op.counts[0].item()), op.mp)
        pk = op.packets.cpu().numpy().view(self.pkg.PACKET_DTYPE)[:nd]
        off = op.offsets.cpu().numpy().view(np.uint32)[: nd + 1]
        arena = op.arena.cpu().numpy()
        for i, p in enumerate(pk):
            if not int(p["open"]):
                s = int(p["shard"])
                self.sent[r][s] = self.sent[r].get(s, b"") + arena[int(off[i]): int(off[i + 1])].tobytes()

    def __call__(self, r, step, op, received, rb, rr, t):
        e, eb, er, ec = self.expectation(r, step)
        label = f"rank {r} launch {step}"
        assert received.astype(np.int64).tolist() == ec.tolist(), label
        got_b = rb.cpu().numpy()
        assert np.array_equal(got_b[: eb.size], eb) and (got_b[eb.size:] == 0xCD).all(), label
        assert np.array_equal(rr.cpu().numpy().view(self.pkg.RECORD_DTYPE)[: len(er)], er), label
        rows = op.all_dead.cpu().numpy().view(np.uint64).reshape(self.world, -1)
        assert np.array_equal(rows, O.dead_rows(self.oracle, self.launches[step], self.n)), (label, rows)
        O.check_owner(self.pkg, op, e, label)
        self.collect(r, op)
        self.expect[(r, step)] = e
        self.fills[r], self.pend[r] = [int(f) for f in e.fill_out], dict(e.new_pending)


# ---- 1. one rank -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 16, 100])
def test_one_rank_matches_oracle(pkg, oracle, n):
    alive = [int(k % 3 != 1) for k in range(n)]
    launches = [[O.rank_inputs(pkg, oracle, 0, 1, n, seed=100 + n, alive=alive)]]
    fills, pend = _state(n, 7 + n)
    ck = _Checker(pkg, oracle, n, launches, [fills], [pend])
    O.run_ranks(pkg, n, launches, [fills], [pend], ck)
    e = ck.expect[(0, 0)]
    assert e.n_lines > 0 and len(e.packets) > 0
    if n >= 3:   # some pending buffers were dropped, others carried into a packet
        assert e.dead and any(fills[s] for s in e.dead)
        assert (e.packets["carry"] > 0).any()


# ---- 2. ranks as threads -----------------------------------------------------------------------------
@pytest.mark.parametrize("world,n", [(2, 16), (2, 64), (3, 16), (3, 64)])
def test_ranks_as_threads_match_oracle(pkg, oracle, world, n):
    launches = [[O.rank_inputs(pkg, oracle, r, world, n, seed=300 + 10 * world + n) for r in range(world)]]
    states = [_state(n, 31 * world + n + r) for r in range(world)]
    fills, pend = [s[0] for s in states], [s[1] for s in states]
    ck = _Checker(pkg, oracle, n, launches, fills, pend)
    calls = O.run_ranks(pkg, n, launches, fills, pend, ck)
    counts = {r: O.expected_receive(oracle, launches[0], world, r)[2] for r in range(world)}
    # rank 0 sends nothing; rank 1 receives nothing; some rank's own chunk is empty while others send to it
    assert all(int(counts[r][0, 0]) == 0 for r in range(world))
    e1 = ck.expect[(1, 0)]
    assert e1.n_lines == 0 and len(e1.packets) == 0 and np.array_equal(e1.fill_out, e1.fill_eff)
    assert e1.dead and any(fills[1][s] for s in e1.dead) and e1.fill_out.any()
    own_empty = [r for r in range(world) if int(counts[r][r, 0]) == 0 and int(counts[r][:, 0].sum()) > 0]
    assert own_empty or world == 2
    assert any(ck.expect[(r, 0)].n_lines > 0 for r in range(world))
    # the bitmap rows travel under tag 2: one group, a send to and a receive from every peer in rank order
    row = 8 * max((n + 63) // 64, 1)
    for r in range(world):
        tagged = [c for c in calls[r] if isinstance(c, tuple) and c[2] == 2]
        assert tagged == [(kind, q, 2, row) for q in range(world) if q != r for kind in ("send", "recv")], (r, tagged)
        first = calls[r].index(tagged[0])
        assert calls[r][first - 1] == "group_start" and calls[r][first + len(tagged)] == "group_end"


# ---- 3. differing snapshots --------------------------------------------------------------------------
def test_drop_comes_before_a_newer_snapshot_s_lines(pkg, oracle):
    """Rank 0 routes with shard k dead (and probes it), rank 1 routes the same bytes with k alive. k's
    owner loses k's old pending bytes and keeps rank 1's lines, packed with carry 0. Handing the ORed
    bitmap to the packing as its probed-dead bitmap would give fill_out[k] = 0 instead."""
    world, n = 2, 4
    datas = [O.batch_bytes(pkg, 900 + b, 4096 + 1000 * b) for b in range(2)]
    all_alive = oracle.route(datas[0], n)[0]
    k = int(all_alive["route"][all_alive["route"] < n][0])
    inputs = []
    for alive in ([int(s != k) for s in range(n)], [1] * n):
        inputs.append((datas, [oracle.route(d, n, alive)[0] for d in datas], alive))
    launches = [inputs]
    owner = k % world
    fills = [[700] * n for _ in range(world)]
    pend = [X.random_pending(np.random.default_rng(5 + r), fills[r]) for r in range(world)]
    ck = _Checker(pkg, oracle, n, launches, fills, pend)
    O.run_ranks(pkg, n, launches, fills, pend, ck)
    assert k in O.source_dead(oracle, inputs[0], n) and k not in O.source_dead(oracle, inputs[1], n)
    e = ck.expect[(owner, 0)]
    mine = e.packets[e.packets["shard"] == k]
    assert len(mine) and int(mine[0]["carry"]) == 0 and int(e.fill_out[k]) > 0
    old = pend[owner][k]
    assert old not in ck.sent[owner].get(k, b"") and not e.new_pending[k].startswith(old)
    lines_k = b"".join(e.bytes[int(r["offset"]): int(r["offset"]) + int(r["length"])].tobytes()
                       for r in e.recs if int(r["route"]) == k)
    assert ck.sent[owner].get(k, b"") + e.new_pending[k] == lines_k
    wrong = oracle.pack_packets(e.recs, n, fills[owner], (k,))[2]
    assert int(wrong[k]) == 0 != int(e.fill_out[k])


# ---- 4. two launches chained on the device, then the flush -------------------------------------------
def test_two_launches_chain_then_flush(pkg, oracle):
    world, n = 3, 16
    launches = [[O.rank_inputs(pkg, oracle, r, world, n, seed=500 + 50 * step) for r in range(world)]
                for step in range(2)]
    states = [_state(n, 77 + r) for r in range(world)]
    fills, pend = [s[0] for s in states], [s[1] for s in states]
    ck = _Checker(pkg, oracle, n, launches, fills, pend)
    flushed = {}

    def finish(r, op, router):
        f = O.FlushExpect(pkg, n, ck.fills[r], ck.pend[r], op.mp, op.pcap)
        op.flush()
        router.sync()
        O.check_flush(pkg, op, f, f"rank {r} flush")
        assert not op.fill[op.cur].cpu().numpy().any()
        ck.collect(r, op)
        flushed[r] = f

    O.run_ranks(pkg, n, launches, fills, pend, ck, finish=finish)
    for r in range(world):
        dropped = set(ck.expect[(r, 0)].dead) | set(ck.expect[(r, 1)].dead)
        for s in range(n):
            # the oracle's materialize chain: launch 0's packets, launch 1's, then what the flush sends
            want = b"".join(b"".join(ck.expect[(r, step)].flushed.get(s, [])) for step in range(2))
            want += flushed[r].sent.get(s, b"")
            assert ck.sent[r].get(s, b"") == want, (r, s)
            if s not in dropped:   # and, where nothing was dropped, simply everything in arrival order
                lines = b"".join(
                    e.bytes[int(x["offset"]): int(x["offset"]) + int(x["length"])].tobytes()
                    for e in (ck.expect[(r, 0)], ck.expect[(r, 1)]) for x in e.recs if int(x["route"]) == s)
                assert want == pend[r][s] + lines, (r, s)
    assert any(ck.expect[(r, 1)].n_lines and (ck.expect[(r, 1)].packets["carry"] > 0).any() for r in range(world))


# ---- 5. sr_flush_pending alone -----------------------------------------------------------------------
def _flush_fills(rng, n):
    fills = rng.choice([0, 1, 1449, 1450], n).astype(np.int64)
    some = rng.random(n) < 0.4
    fills[some] = rng.integers(0, 1451, int(some.sum()))
    if n >= 7:
        fills[:5] = [1450, 0, 1, 1449, 0]
    else:
        fills[0] = 1449
    return fills.tolist()


@pytest.mark.parametrize("n", [1, 7, 64, 4096])
def test_flush_pending_alone(pkg, oracle, torch_stream, n):
    import importlib

    import torch

    rg = importlib.import_module("statsd-router_amd.regroup")
    rng = np.random.default_rng(1000 + n)
    fills = _flush_fills(rng, n)
    pend = X.random_pending(rng, fills)
    need = sum(fills)
    count = sum(1 for f in fills if f)
    with pkg.Router(n, 4096) as r:
        r.set_stream(torch_stream.cuda_stream)
        # (max_packets, payload_cap, bytes in front of the arena): enough room; an odd arena base with the
        # arena one byte short; descriptor room one short
        for mp, cap, lead in [(n, pkg.payload_capacity(0, n), 0), (n, need - 1, 3), (count - 1, need, 1)]:
            op = rg.OwnerPacker(pkg, r, 1, 1, 0, max_packets=mp, payload_cap=cap, poison=O.POISON)
            whole = torch.full((lead + cap + op.slack,), O.POISON, dtype=torch.uint8, device="cuda")
            op.arena = whole[lead:]
            op.set_pending(fills, X.pending_image(pend, n, fills))
            e = O.FlushExpect(pkg, n, fills, pend, mp, cap)
            op.flush()
            torch.cuda.synchronize()
            label = f"n {n} max_packets {mp} cap {cap} lead {lead}"
            O.check_flush(pkg, op, e, label)
            assert (whole[:lead].cpu().numpy() == O.POISON).all(), label
            assert (op.pend[op.cur].cpu().numpy() == X.pending_image(pend, n, fills)).all(), label
            if cap == need - 1:     # the last packet is cut: reported, its fill kept
                last = max(s for s in range(n) if fills[s])
                assert int(op.total.item()) == need > cap and e.fill_after[last] == fills[last]
                assert sum(1 for s in range(n) if e.fill_after[s]) == 1
            if mp == count - 1:
                assert int(op.counts[0].item()) == count > mp and sum(1 for s in range(n) if e.fill_after[s]) == 1
            # flushing what is left with enough room sends the rest and nothing twice
            if e.fill_after.any():
                left = e.fill_after.tolist()
                e2 = O.FlushExpect(pkg, n, left, pend, n, pkg.payload_capacity(0, n))
                op2 = rg.OwnerPacker(pkg, r, 1, 1, 0, max_packets=n, poison=O.POISON)
                op2.fill, op2.pend, op2.cur = op.fill, op.pend, op.cur
                op2.flush()
                torch.cuda.synchronize()
                O.check_flush(pkg, op2, e2, label + " (again)")
                assert {**e.sent, **e2.sent} == {s: pend[s][: fills[s]] for s in range(n) if fills[s]}


def test_flush_pending_under_capture(pkg, oracle, torch_stream):
    """No scratch: sr_flush_pending is captured as it is, and replayed on other pending bytes."""
    import importlib

    import torch

    rg = importlib.import_module("statsd-router_amd.regroup")
    n = 64
    rng = np.random.default_rng(2024)
    with pkg.Router(n, 4096) as r:
        r.set_stream(torch_stream.cuda_stream)
        op = rg.OwnerPacker(pkg, r, 1, 1, 0, max_packets=n, poison=O.POISON)
        op.flush()   # warm: the kernels' code is loaded outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch_stream):
            r.flush_pending(op.fill[0].data_ptr(), op.pend[0].data_ptr(), op.packets.data_ptr(), op.mp,
                            op.counts.data_ptr(), op.arena.data_ptr(), op.pcap, op.offsets.data_ptr(),
                            op.total.data_ptr())
        for _ in range(2):
            fills = _flush_fills(rng, n)
            pend = X.random_pending(rng, fills)
            op.set_pending(fills, X.pending_image(pend, n, fills))
            op._refill(op.packets, op.counts, op.arena, op.offsets, op.total)
            g.replay()
            torch.cuda.synchronize()
            O.check_flush(pkg, op, O.FlushExpect(pkg, n, fills, pend, op.mp, op.pcap), "replay")


# ---- 6. room -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["max_packets", "payload_cap"])
def test_owner_pack_room_one_short(pkg, oracle, short):
    """Descriptor room or arena room one short: reported as sr_pack_packets / sr_pack_payloads report it
    (d_counts[0] > max_packets, *d_total > payload_cap), what fits is right, nothing past it is written."""
    n = 16
    alive = [int(k % 3 != 1) for k in range(n)]
    launches = [[O.rank_inputs(pkg, oracle, 0, 1, n, seed=640, alive=alive)]]
    fills, pend = _state(n, 99)
    e = _Checker(pkg, oracle, n, launches, [fills], [pend]).expectation(0, 0)[0]
    room = {"max_packets": len(e.packets) - 1} if short == "max_packets" else {"payload_cap": e.total - 1}
    seen = {}

    def check(r, step, op, received, rb, rr, t):
        O.check_owner(pkg, op, e, short)
        seen["counts"], seen["total"], seen["mp"], seen["pcap"] = int(op.counts[0].item()), int(op.total.item()), op.mp, op.pcap

    O.run_ranks(pkg, n, launches, [fills], [pend], check, packer=room)
    if short == "max_packets":
        assert seen["counts"] == len(e.packets) > seen["mp"]
    else:
        assert seen["total"] == e.total > seen["pcap"]


# ---- 7. argument errors ------------------------------------------------------------------------------
def test_argument_errors(pkg, oracle, torch_stream):
    import torch

    n = 4
    z = lambda k, dt=torch.int64: torch.zeros(k, dtype=dt, device="cuda")
    with pkg.Router(n, 4096) as r:
        r.set_stream(torch_stream.cuda_stream)
        rb, rr, rc = z(4096, torch.uint8), z(512), z(2)
        srt, pk, cnt, fout = z(512), z(2 * 64), z(3), z(n, torch.int16)
        pin, pout = z(n * pkg.PENDING_STRIDE, torch.uint8), z(n * pkg.PENDING_STRIDE, torch.uint8)
        arena, off, tot = z(1 << 14, torch.uint8), z(65, torch.int32), z(1)
        good = dict(d_recv_bytes=rb.data_ptr(), recv_nbytes=4096, d_recv_recs=rr.data_ptr(), max_records=512,
                    d_recv_counts=rc.data_ptr(), world=1, d_sorted=srt.data_ptr(), d_packets=pk.data_ptr(),
                    max_packets=64, d_counts=cnt.data_ptr(), d_fill_out=fout.data_ptr(), d_pend_in=pin.data_ptr(),
                    d_pend_out=pout.data_ptr(), d_payload=arena.data_ptr(), payload_cap=1 << 14,
                    d_offsets=off.data_ptr(), d_total=tot.data_ptr())
        r.owner_pack(**good)   # (nothing received: a valid call)
        r.sync()
        assert cnt.cpu().tolist() == [0, 0, 0] and int(tot.item()) == 0
        bad = [dict(d_recv_counts=0), dict(d_recv_recs=0), dict(d_sorted=0), dict(d_packets=0), dict(d_counts=0),
               dict(d_fill_out=0), dict(d_offsets=0), dict(d_total=0), dict(d_recv_bytes=0),
               dict(d_pend_out=pin.data_ptr()), dict(d_pend_in=0), dict(world=0), dict(world=65)]
        for change in bad:
            with pytest.raises(pkg.SrError) as ei:
                r.owner_pack(**{**good, **change})
            assert ei.value.errno == errno.EINVAL, change
        fl = z(n, torch.int16)
        ok = [fl.data_ptr(), pin.data_ptr(), pk.data_ptr(), 64, cnt.data_ptr(), arena.data_ptr(), 1 << 14,
              off.data_ptr(), tot.data_ptr()]
        r.flush_pending(*ok)
        for i in (0, 1, 2, 4, 5, 7, 8):
            args = list(ok)
            args[i] = 0
            with pytest.raises(pkg.SrError) as ei:
                r.flush_pending(*args)
            assert ei.value.errno == errno.EINVAL, i
        dead = z(1)
        with pytest.raises(pkg.SrError) as ei:
            r.exchange_dead_run(pkg.Transport(), 1, 0, [], 0)
        assert ei.value.errno == errno.EINVAL
        r.exchange_dead_run(pkg.Transport(), 1, 0, [], dead.data_ptr())   # no batch: an empty row, no transport call
        r.sync()
        assert int(dead.item()) == 0


# ---- 8. a one-rank RCCL communicator -----------------------------------------------------------------
def test_one_rank_comm(pkg, oracle):
    """sr_regroup_launch + sr_exchange_dead on a one-rank communicator: row 0 is the launch's ORed bitmap
    (one rank: the C code returns before any send or receive), and the pack equals the oracle."""
    n = 16
    alive = [int(k % 3 != 1) for k in range(n)]
    launches = [[O.rank_inputs(pkg, oracle, 0, 1, n, seed=808, alive=alive)]]
    fills, pend = _state(n, 8)
    ck = _Checker(pkg, oracle, n, launches, [fills], [pend])
    O.run_ranks(pkg, n, launches, [fills], [pend], ck, use_comm=True)
    assert ck.expect[(0, 0)].dead and ck.expect[(0, 0)].n_lines
