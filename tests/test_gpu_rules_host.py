"""GPU: sr_set_name_rules, the name rules of the host-memory path. Double-buffered submissions, slot-2 synchronous
calls, and the switch together with sr_set_coalesce: `sorted`, `packets` and `fill` equal the oracle's packing of
the restatement's kept records (tests/rules_expect.py, then tests/coalesce_expect.py), the counts come back through
sr_route_pack_rules, and the trace and the name statistics are those of the input, as with the switch off."""
from __future__ import annotations

import errno

import numpy as np
import pytest

import coalesce_expect as CE
import payload_expect as X
import rules_expect as E
import stats_expect as S
from rules_expect import DROP, EXACT, KEEP, PREFIX

pytestmark = pytest.mark.gpu

RULES = [(b"debug.", PREFIX, DROP), (b"debug.keep.", PREFIX, KEEP), (b"svc.req.7", EXACT, DROP), (b"host.hot", EXACT, DROP)]


def traffic(seed, count):
    rng = np.random.default_rng(seed)
    lines = []
    for u, k, v in zip(rng.random(count), rng.integers(0, 12, count), rng.integers(1, 500, count)):
        if u < 0.2:
            lines.append(b"host.hot:1|c")
        elif u < 0.4:
            lines.append(b"debug.t%d:%d|c" % (k, v))
        elif u < 0.5:
            lines.append(b"debug.keep.t%d:1|c" % k)
        elif u < 0.85:
            lines.append(b"svc.req.%d:%d|c" % (k, v))
        elif u < 0.92:
            lines.append(b"svc.lat.%d:%d|ms" % (k, v))
        elif u < 0.96:
            lines.append(b"bad")
        else:
            lines.append(b"debug.no colon in this line")
    return b"".join(l + b"\n" for l in lines)


class Want:
    """The oracle's routing, the restatement's rules (and coalescing), the oracle's packing of that."""

    def __init__(self, oracle, data, n, alive, fills, coalesce=False):
        arr = np.frombuffer(data, np.uint8)
        self.recs, self.hashes, self.n_in = oracle.route(arr, n, alive)
        self.probed = oracle.probed_dead(arr, n, alive) if alive is not None else np.zeros(0, np.int64)
        self.res = E.apply(data, self.recs, self.hashes, n, RULES)
        out = self.res.out
        if coalesce:
            self.co = CE.coalesce(data, self.res.out, self.res.hashes_out, n, CE.DEFAULT_SLOTS, len(data))
            out = self.co.out
        self.whole = data + (self.co.text if coalesce else b"")
        self.pack_records(oracle, out, n, fills)

    def pack_records(self, oracle, out, n, fills):
        self.sorted, self.packets, self.fill_out, self.n_valid = oracle.pack_packets(out, n, fills, self.probed)
        pending = {k: bytes(int(f)) for k, f in enumerate(fills)}
        self.arena, self.offsets, self.rooms = X.flat_expectation(self.whole, self.sorted, self.packets, pending)
        self.total = int(self.offsets[-1])

    def pack(self):
        return (self.sorted, self.packets, self.fill_out, self.n_valid, self.probed)


def check_slot(r, slot, w, label, trace, coalesce, payloads=False):
    from test_gpu_mtu import assert_pack_equal
    from test_gpu_payloads import _check_host

    assert_pack_equal(r.route_pack_result(slot), w.pack())
    assert r.route_pack_rules(slot).tolist() == w.res.counts.tolist(), label
    if coalesce:
        text, counts = r.route_pack_coalesced(slot)
        assert text == w.co.text and counts.tolist() == w.co.counts.tolist(), label
    if payloads:
        _check_host(r.route_pack_payloads(slot), w, label)
    if trace:
        recs, hs = r.route_pack_trace(slot)
        assert np.array_equal(recs, w.recs) and np.array_equal(hs, w.hashes), f"{label}: trace"


@pytest.mark.parametrize("trace,coalesce,payloads", [(False, False, False), (True, False, True), (False, True, True),
                                                     (True, True, True), (False, False, True)],
                         ids=["plain", "trace+payloads", "coalesce+payloads", "trace+coalesce+payloads", "payloads"])
def test_double_buffered_and_synchronous_submissions(pkg, oracle, trace, coalesce, payloads):
    n = 6
    rng = np.random.default_rng(5)
    with pkg.Router(n, 1 << 17) as r:
        r.route_pack_submit(0, b"k:1|c\nk:2|c\n")
        r.route_pack_result(0)
        with pytest.raises(pkg.SrError) as ei:   # submitted with the switch off
            r.route_pack_rules(0)
        assert ei.value.errno == errno.EBUSY
        with pytest.raises(pkg.SrError) as ei:   # a bad set leaves the switch off
            r.set_name_rules(pkg.RuleSet([(b"a:b", PREFIX, DROP)]))
        assert ei.value.errno == errno.EINVAL
        r.set_name_rules(pkg.RuleSet(RULES))
        r.set_coalesce(coalesce)
        r.set_trace(trace)
        r.set_payloads(payloads)
        r.set_name_stats(True)
        fill_o = [0] * n
        inflight = None
        dropped = 0
        every = []
        for b in range(7):
            alive = (rng.random(n) > 0.25).astype(int).tolist() if b % 3 else None
            data = traffic(40 + b, int(rng.integers(1, 3000))) if b != 5 else b""
            every.append((data, alive))
            host_fill = None
            if b in (0, 4):
                host_fill = rng.integers(0, 1451, n).tolist()
                if inflight is not None:
                    check_slot(r, *inflight, trace, coalesce, payloads)
                    inflight = None
                fill_o = host_fill
            r.set_alive(alive if alive is not None else [1] * n)
            slot = b % 2
            r.route_pack_submit(slot, data, host_fill)
            with pytest.raises(pkg.SrError) as ei:   # in flight
                r.route_pack_rules(slot)
            assert ei.value.errno == errno.EBUSY
            w = Want(oracle, data, n, alive, fill_o, coalesce)
            dropped += int(w.res.counts[1])
            fill_o = [int(f) for f in w.fill_out]
            if inflight is not None:
                check_slot(r, *inflight, trace, coalesce, payloads)
            inflight = (slot, w, f"batch {b}")
        check_slot(r, *inflight, trace, coalesce, payloads)
        assert dropped > 100
        # slot 2: the synchronous call
        data = traffic(99, 2500)
        every.append((data, alive))
        w = Want(oracle, data, n, alive, fill_o, coalesce)
        srt, pk, fo, nv, pr = r.route_pack(data, fill_o)
        assert np.array_equal(srt, w.sorted) and np.array_equal(pk.view(np.uint8), w.packets.view(np.uint8))
        assert nv == w.n_valid and [int(f) for f in fo] == [int(f) for f in w.fill_out]
        assert r.route_pack_rules(2).tolist() == w.res.counts.tolist()
        hits = r.rules_read()
        assert int(hits[:, 0].sum()) > 0 and int(hits[0, 0] + hits[2, 0] + hits[3, 0]) == dropped + int(w.res.counts[1])
        # the name statistics saw every input line, the dropped ones included: the switch off gives the same
        got = r.stats_read()
        r.set_name_rules(None)
        r.set_coalesce(False)
    with pkg.Router(n, 1 << 17) as r2:
        r2.set_name_stats(True)
        for data, alive in every:
            r2.set_alive(alive if alive is not None else [1] * n)
            r2.route_pack(data, [0] * n)
        assert S.same(got, r2.stats_read()) == []


@pytest.mark.parametrize("coalesce", [False, True], ids=["rules", "rules+coalesce"])
def test_slot_submissions(pkg, oracle, coalesce):
    """sr_route_pack_submit_slots with the switch on: the datagrams are framed on the device, then the rules run,
    with payloads and trace."""
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
        r.set_name_rules(pkg.RuleSet(RULES))
        r.set_coalesce(coalesce)
        r.set_payloads(True)
        r.set_trace(True)
        r.route_pack_submit_slots(0, buf, 4096, lens, [0] * n)
        w = Want(oracle, data, n, None, [0] * n, coalesce)
        check_slot(r, 0, w, "slots", True, coalesce, True)
        assert int(w.res.counts[1]) > 1000


def test_logs_and_statistics_are_those_of_the_switch_off(pkg, oracle):
    """The log text at TRACE level (it reads the input-order records, the hashes and the datagram ends), the trace
    and the name statistics, byte for byte, with the switch off and on; slot submissions and plain ones."""
    import frame_slots as F

    n = 5
    dgrams = [traffic(300 + i, 30)[:-1] for i in range(40)]
    arena, lens = F.build_arena(dgrams, 4096)
    outs = []
    for on in (False, True):
        with pkg.Router(n, 1 << 17) as r:
            r.set_logtext(pkg.SR_LOG_TRACE)
            r.set_name_stats(True, hll_p=6, cms_rows=3, cms_width=256, hot_slots=16, hot_div=8, hot_min_lines=2)
            r.set_trace(True)
            if on:
                r.set_name_rules(pkg.RuleSet(RULES))
            buf = pkg.HostBuffer(arena.size)
            buf.array[:] = arena
            got = []
            for b in range(4):
                r.route_pack_set_prefix(b % 2, b"T%d " % b, b"W%d " % b)
                if b == 3:
                    r.route_pack_submit_slots(b % 2, buf, 4096, lens, None)
                else:
                    r.route_pack_submit(b % 2, traffic(70 + b, 1500), [0] * n if b == 0 else None)
                r.route_pack_result(b % 2)
                got.append((r.route_pack_logtext(b % 2), r.route_pack_trace(b % 2)))
            if on:
                assert int(r.route_pack_rules(1)[1]) > 100
            snap = r.stats_read()
            outs.append((got, snap))
    for (la, ta), (lb, tb) in zip(outs[0][0], outs[1][0]):
        assert la[0] == lb[0] and la[1] == lb[1] and np.array_equal(la[2], lb[2]) and np.array_equal(la[3], lb[3])
        assert len(la[0]) > 1000
        assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])
    a, b = outs[0][1], outs[1][1]
    assert np.array_equal(a.lines, b.lines) and np.array_equal(a.cells, b.cells) and np.array_equal(a.regs, b.regs)
    assert np.array_equal(a.hot, b.hot) and a.n_hot > 0


def test_argument_errors_and_busy(pkg):
    lib = pkg.lib()
    with pkg.Router(2, 1 << 16) as r:
        assert lib.sr_set_name_rules(None, None) == -errno.EINVAL
        r.set_name_rules(pkg.RuleSet([(b"a.", PREFIX, DROP)]))
        r.route_pack_submit(0, b"a.b:1|c\nc.d:2|c\n")
        for call in (lambda: r.set_name_rules(None), lambda: r.set_name_rules(pkg.RuleSet([])), r.rules_close):
            with pytest.raises(pkg.SrError) as ei:   # a slot is in flight
                call()
            assert ei.value.errno == errno.EBUSY
        srt, pk, fill, nv, _ = r.route_pack_result(0)
        assert len(srt) == 1 and int(srt[0]["offset"]) == 8 and nv == 1
        assert r.route_pack_rules(0).tolist() == [1, 1, 8, 2]
        r.route_pack_submit(1, b"")                    # an empty batch with the switch on
        r.route_pack_result(1)
        assert r.route_pack_rules(1).tolist() == [0, 0, 0, 0]
        r.set_name_rules(pkg.RuleSet([(b"c.", PREFIX, DROP)]))   # a new set replaces the old one, hits included
        assert r.rules_read().tolist() == [[0, 0], [0, 0]]
        r.route_pack_submit(0, b"a.b:1|c\nc.d:2|c\n")
        assert int(r.route_pack_result(0)[0][0]["offset"]) == 0
        r.rules_close()                                # the switch goes with the stage
        r.route_pack_submit(0, b"a.b:1|c\nc.d:2|c\n")
        assert len(r.route_pack_result(0)[0]) == 2
