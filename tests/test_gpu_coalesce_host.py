"""GPU: sr_set_coalesce, the coalescing of the host-memory path. Double-buffered submissions, slot submissions
and the synchronous call with the switch on: `sorted`, `packets`, `fill` and the payloads equal the oracle's
packing of the restatement's coalesced records (tests/coalesce_expect.py), the merged text and the counts come
back through sr_route_pack_coalesced, and the trace, the log text and the name statistics are those of the same
session with the switch off."""
from __future__ import annotations

import errno

import numpy as np
import pytest

import coalesce_expect as E
import payload_expect as X

pytestmark = pytest.mark.gpu


def traffic(seed, count, hot=0.4):
    """A framed batch: a hot counter, a pool of counters, timers, sampled counters and invalid lines."""
    rng = np.random.default_rng(seed)
    lines = []
    for u, k, v in zip(rng.random(count), rng.integers(0, 30, count), rng.integers(1, 500, count)):
        if u < hot:
            lines.append(b"host.hot:1|c")
        elif u < 0.75:
            lines.append(b"svc.req.%d:%d|c" % (k, v))
        elif u < 0.85:
            lines.append(b"svc.lat.%d:%d|ms" % (k, v))
        elif u < 0.92:
            lines.append(b"svc.req.%d:%d|c|@0.1" % (k, v))
        elif u < 0.96:
            lines.append(b"bad")
        else:
            lines.append(b"no colon in this line")
    return b"".join(l + b"\n" for l in lines)


class Want:
    """The oracle's routing, the restatement's coalescing, the oracle's packing of that."""

    def __init__(self, oracle, data, n, alive, fills):
        arr = np.frombuffer(data, np.uint8)
        self.recs, self.hashes, self.n_in = oracle.route(arr, n, alive)
        self.probed = oracle.probed_dead(arr, n, alive) if alive is not None else np.zeros(0, np.int64)
        self.res = E.coalesce(data, self.recs, self.hashes, n, E.DEFAULT_SLOTS, len(data))
        assert self.res.complete
        self.whole = data + self.res.text
        self.sorted, self.packets, self.fill_out, self.n_valid = oracle.pack_packets(self.res.out, n, fills, self.probed)
        pending = {k: bytes(int(f)) for k, f in enumerate(fills)}
        self.arena, self.offsets, self.rooms = X.flat_expectation(self.whole, self.sorted, self.packets, pending)
        self.total = int(self.offsets[-1])

    def pack(self):
        return (self.sorted, self.packets, self.fill_out, self.n_valid, self.probed)


def check_slot(r, slot, w, label, payloads, trace):
    from test_gpu_mtu import assert_pack_equal
    from test_gpu_payloads import _check_host

    assert_pack_equal(r.route_pack_result(slot), w.pack())
    text, counts = r.route_pack_coalesced(slot)
    assert text == w.res.text and counts.tolist() == w.res.counts.tolist(), label
    if payloads:
        _check_host(r.route_pack_payloads(slot), w, label)
    if trace:
        recs, hs = r.route_pack_trace(slot)
        assert np.array_equal(recs, w.recs) and np.array_equal(hs, w.hashes), f"{label}: trace"


@pytest.mark.parametrize("payloads,trace", [(False, False), (True, False), (True, True)],
                         ids=["plain", "payloads", "payloads+trace"])
def test_double_buffered_submissions(pkg, oracle, payloads, trace):
    n = 6
    rng = np.random.default_rng(5)
    with pkg.Router(n, 1 << 17) as r:
        r.route_pack_submit(0, b"k:1|c\nk:2|c\n")
        r.route_pack_result(0)
        with pytest.raises(pkg.SrError) as ei:   # submitted with the switch off
            r.route_pack_coalesced(0)
        assert ei.value.errno == errno.EBUSY
        r.set_coalesce(True)
        r.set_payloads(payloads)
        r.set_trace(trace)
        fill_o = [0] * n
        inflight = None
        merged = 0
        for b in range(8):
            alive = (rng.random(n) > 0.25).astype(int).tolist() if b % 3 else None
            data = traffic(40 + b, int(rng.integers(1, 4000)), hot=0.5 if b != 4 else 0.0) if b != 5 else b""
            host_fill = None
            if b in (0, 4):
                host_fill = rng.integers(0, 1451, n).tolist()
                if inflight is not None:
                    check_slot(r, *inflight, payloads, trace)
                    inflight = None
                fill_o = host_fill
            r.set_alive(alive if alive is not None else [1] * n)
            slot = b % 2
            r.route_pack_submit(slot, data, host_fill)
            with pytest.raises(pkg.SrError) as ei:   # in flight
                r.route_pack_coalesced(slot)
            assert ei.value.errno == errno.EBUSY
            w = Want(oracle, data, n, alive, fill_o)
            merged += int(w.res.counts[2])
            fill_o = [int(f) for f in w.fill_out]
            if inflight is not None:
                check_slot(r, *inflight, payloads, trace)
            inflight = (slot, w, f"batch {b}")
        check_slot(r, *inflight, payloads, trace)
        assert merged > 50
        # slot 2: the synchronous call
        data = traffic(99, 3000)
        w = Want(oracle, data, n, alive, fill_o)
        srt, pk, fo, nv, pr = r.route_pack(data, fill_o)
        assert np.array_equal(srt, w.sorted) and np.array_equal(pk.view(np.uint8), w.packets.view(np.uint8))
        assert nv == w.n_valid and [int(f) for f in fo] == [int(f) for f in w.fill_out]
        text, counts = r.route_pack_coalesced(2)
        assert text == w.res.text and counts.tolist() == w.res.counts.tolist()
        assert b"host.hot:%d|c\n" % data.count(b"host.hot:1|c\n") in text
        # off again: the parent's path, and the accessor says so
        r.set_coalesce(False)
        e = X.Expect(oracle, data, n, alive, fill_o, {k: bytes(int(f)) for k, f in enumerate(fill_o)})
        srt, pk, fo, nv, pr = r.route_pack(data, fill_o)
        assert np.array_equal(srt, e.sorted) and np.array_equal(pk.view(np.uint8), e.packets.view(np.uint8))
        with pytest.raises(pkg.SrError) as ei:
            r.route_pack_coalesced(2)
        assert ei.value.errno == errno.EBUSY


def test_slot_submissions(pkg, oracle):
    """sr_route_pack_submit_slots with the switch on: the datagrams are framed on the device, then coalesced."""
    import frame_slots as F

    n = 4
    rng = np.random.default_rng(8)
    dgrams = [traffic(200 + i, int(rng.integers(1, 40)))[:-1] for i in range(300)]   # no '\n' at the end: framed
    dgrams[7] = b"host.hot:1|c\n" * 50 + b"other.line:3|ms\n"
    data = b"".join(d if d.endswith(b"\n") else d + b"\n" for d in dgrams)
    arena, lens = F.build_arena(dgrams, 4096)
    buf = pkg.HostBuffer(arena.size)
    buf.array[:] = arena
    with pkg.Router(n, 1 << 18) as r:
        r.set_coalesce(True, slots=1 << 12)
        r.route_pack_submit_slots(0, buf, 4096, lens, [0] * n)
        w = Want(oracle, data, n, None, [0] * n)
        w.res = E.coalesce(data, w.recs, w.hashes, n, 1 << 12, len(data))
        w.sorted, w.packets, w.fill_out, w.n_valid = oracle.pack_packets(w.res.out, n, [0] * n, w.probed)
        check_slot(r, 0, w, "slots", False, False)
        assert int(w.res.counts[1]) > 1000


def test_logs_and_statistics_are_those_of_the_switch_off(pkg, oracle):
    n = 5
    outs = []
    for on in (False, True):
        with pkg.Router(n, 1 << 17) as r:
            r.set_logtext(pkg.SR_LOG_TRACE)
            r.set_name_stats(True, hll_p=6, cms_rows=3, cms_width=256, hot_slots=16, hot_div=8, hot_min_lines=2)
            r.set_trace(True)
            if on:
                r.set_coalesce(True)
            got = []
            for b in range(3):
                data = traffic(70 + b, 1500)
                r.route_pack_set_prefix(b % 2, b"T%d " % b, b"W%d " % b)
                r.route_pack_submit(b % 2, data, [0] * n if b == 0 else None)
                r.route_pack_result(b % 2)
                got.append((r.route_pack_logtext(b % 2), r.route_pack_trace(b % 2)))
            snap = r.stats_read()
            outs.append((got, snap))
    for (la, ta), (lb, tb) in zip(outs[0][0], outs[1][0]):
        assert la[0] == lb[0] and la[1] == lb[1] and np.array_equal(la[2], lb[2]) and np.array_equal(la[3], lb[3])
        assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])
    a, b = outs[0][1], outs[1][1]
    assert np.array_equal(a.lines, b.lines) and np.array_equal(a.cells, b.cells) and np.array_equal(a.regs, b.regs)
    assert np.array_equal(a.hot, b.hot) and a.n_hot > 0


def test_argument_errors_and_busy(pkg):
    lib = pkg.lib()
    with pkg.Router(2, 1 << 16) as r:
        assert lib.sr_set_coalesce(None, None) == -errno.EINVAL
        with pytest.raises(pkg.SrError) as ei:
            r.set_coalesce(True, slots=24)
        assert ei.value.errno == errno.EINVAL
        r.set_coalesce(True, slots=16)
        r.route_pack_submit(0, b"a.b:1|c\na.b:2|c\n")
        for call in (lambda: r.set_coalesce(False), lambda: r.set_coalesce(True), r.coalesce_close):
            with pytest.raises(pkg.SrError) as ei:   # a slot is in flight
                call()
            assert ei.value.errno == errno.EBUSY
        srt, pk, fill, nv, _ = r.route_pack_result(0)
        assert len(srt) == 1 and int(srt[0]["offset"]) == 16 and nv == 1
        text, counts = r.route_pack_coalesced(0)
        assert text == b"a.b:3|c\n" and counts.tolist() == [1, 1, 1, 8]
        r.route_pack_submit(1, b"")                    # an empty batch with the switch on
        r.route_pack_result(1)
        assert r.route_pack_coalesced(1)[1].tolist() == [0, 0, 0, 0]
        r.coalesce_close()                             # the switch goes with the stage
        r.route_pack_submit(0, b"a.b:1|c\na.b:2|c\n")
        assert len(r.route_pack_result(0)[0]) == 2
    with pkg.Router(2, (1 << 30) + 16) as big:         # no room for the text behind such a batch
        with pytest.raises(pkg.SrError) as ei:
            big.set_coalesce(True)
        assert ei.value.errno == errno.EINVAL
