"""GPU: sr_set_validate, the line grammar of the host-memory path, in double-buffered, slot and synchronous
submissions, each crossed with the name rules on/off and the coalescing on/off: twelve submissions on one context.
`sorted`, `packets` and `fill` equal the oracle's packing of the restatements composed in the order route, validate,
rules, coalesce (tests/validate_expect.py, tests/rules_expect.py, tests/coalesce_expect.py); the counts come back
through sr_route_pack_validate; the trace, the log text and the name statistics are those of the switch off; a
toggle with a slot in flight is -EBUSY."""
from __future__ import annotations

import errno

import numpy as np
import pytest

import coalesce_expect as CE
import rules_expect as RE
import validate_expect as E
from test_gpu_rules_host import RULES, Want, check_slot

pytestmark = pytest.mark.gpu

DROP = (1 << E.VALUE) | (1 << E.TYPE) | (1 << E.NO_TYPE) | (1 << E.RATE) | (1 << E.TAGS) | (1 << E.SECTION)


def traffic(seed, count):
    rng = np.random.default_rng(seed)
    kinds = [b"host.hot:1|c", b"host.hot:2|c", b"debug.t%d:%d|c", b"svc.req.%d:%d|c", b"svc.lat.%d:%d|ms|@0.5", b"svc.g.%d:+%d|g",
             b"svc.bad.%d:x%d|c", b"debug.bad.%d:%d|q", b"host.hot:1|c|@x", b"svc.nt.%d:%d", b"svc.tag.%d:%d|c|#", b"bad",
             b"no colon in this line", b"svc.req.7:1|c|#a:b"]
    lines = []
    for k, a, v in zip(rng.integers(0, len(kinds), count), rng.integers(0, 9, count), rng.integers(1, 500, count)):
        f = kinds[k]
        lines.append(f % (a, v) if b"%d" in f else f)
    return b"".join(l + b"\n" for l in lines)


class WantV(Want):
    """The oracle's routing, then the restatements in the submit paths' order, then the oracle's packing."""

    def __init__(self, oracle, data, n, alive, fills, rules, coalesce):
        arr = np.frombuffer(data, np.uint8)
        self.recs, self.hashes, self.n_in = oracle.route(arr, n, alive)
        self.probed = oracle.probed_dead(arr, n, alive) if alive is not None else np.zeros(0, np.int64)
        self.v = E.apply(data, self.recs, self.hashes, n, DROP)
        out, hs = self.v.out, self.v.hashes_out
        if rules:
            self.res = RE.apply(data, out, hs, n, RULES)
            out, hs = self.res.out, self.res.hashes_out
        if coalesce:
            self.co = CE.coalesce(data, out, hs, n, CE.DEFAULT_SLOTS, len(data))
            out = self.co.out
        self.whole = data + (self.co.text if coalesce else b"")
        self.pack_records(oracle, out, n, fills)


def check(r, slot, w, label, rules, coalesce):
    from test_gpu_mtu import assert_pack_equal
    from test_gpu_payloads import _check_host

    assert_pack_equal(r.route_pack_result(slot), w.pack())
    assert r.route_pack_validate(slot).tolist() == w.v.counts.tolist(), label
    if rules:
        assert r.route_pack_rules(slot).tolist() == w.res.counts.tolist(), label
    if coalesce:
        text, counts = r.route_pack_coalesced(slot)
        assert text == w.co.text and counts.tolist() == w.co.counts.tolist(), label
    _check_host(r.route_pack_payloads(slot), w, label)
    recs, hs = r.route_pack_trace(slot)
    assert np.array_equal(recs, w.recs) and np.array_equal(hs, w.hashes), f"{label}: trace"


def test_twelve_submissions_on_one_context(pkg, oracle):
    import frame_slots as F

    n = 5
    rng = np.random.default_rng(17)
    hits = np.zeros((E.REASONS, 2), np.uint64)
    with pkg.Router(n, 1 << 18) as r:
        r.route_pack_submit(0, b"k:1|c\nk:2|c\n")
        r.route_pack_result(0)
        with pytest.raises(pkg.SrError) as ei:   # submitted with the switch off
            r.route_pack_validate(0)
        assert ei.value.errno == errno.EBUSY
        with pytest.raises(pkg.SrError) as ei:   # a bad configuration leaves the switch off
            r.set_validate(pkg.ValidateConfig(1))
        assert ei.value.errno == errno.EINVAL
        r.set_validate(pkg.ValidateConfig(DROP))
        r.set_trace(True)
        r.set_payloads(True)
        fill = [0] * n
        k = 0
        for rules in (False, True):
            for coalesce in (False, True):
                r.set_name_rules(pkg.RuleSet(RULES) if rules else None)
                r.set_coalesce(coalesce)
                for path in ("submit", "slots", "batch"):
                    k += 1
                    label = f"{path} rules={rules} coalesce={coalesce}"
                    alive = (rng.random(n) > 0.25).astype(int).tolist() if k % 3 == 0 else None
                    r.set_alive(alive if alive is not None else [1] * n)
                    if path == "slots":
                        dgrams = [traffic(500 + 40 * k + i, int(rng.integers(1, 30)))[:-1] for i in range(60)]
                        data = b"".join(d + b"\n" for d in dgrams)
                        arena, lens = F.build_arena(dgrams, 4096)
                        buf = pkg.HostBuffer(arena.size)
                        buf.array[:] = arena
                        r.route_pack_submit_slots(k % 2, buf, 4096, lens, fill)
                        with pytest.raises(pkg.SrError) as ei:   # a toggle with a slot in flight
                            r.set_validate(None)
                        assert ei.value.errno == errno.EBUSY
                        w = WantV(oracle, data, n, alive, fill, rules, coalesce)
                        check(r, k % 2, w, label, rules, coalesce)
                    elif path == "submit":
                        data = traffic(100 + k, int(rng.integers(300, 900)))
                        r.route_pack_submit(k % 2, data, fill)
                        with pytest.raises(pkg.SrError) as ei:
                            r.route_pack_validate(k % 2)
                        assert ei.value.errno == errno.EBUSY
                        w = WantV(oracle, data, n, alive, fill, rules, coalesce)
                        check(r, k % 2, w, label, rules, coalesce)
                    else:
                        data = traffic(100 + k, int(rng.integers(300, 900)))
                        w = WantV(oracle, data, n, alive, fill, rules, coalesce)
                        srt, pk, fo, nv, pr = r.route_pack(data, fill)
                        assert np.array_equal(srt, w.sorted) and np.array_equal(pk.view(np.uint8), w.packets.view(np.uint8)), label
                        assert nv == w.n_valid and [int(f) for f in fo] == [int(f) for f in w.fill_out], label
                        assert r.route_pack_validate(2).tolist() == w.v.counts.tolist(), label
                        if rules:
                            assert r.route_pack_rules(2).tolist() == w.res.counts.tolist(), label
                    assert int(w.v.counts[1]) > 20, label
                    hits += w.v.hits
                    fill = [int(f) for f in w.fill_out]
        assert k == 12 and r.validate_read().tolist() == hits.tolist()
        r.validate_close()                                 # the switch goes with the stage
        r.set_name_rules(None)
        r.set_coalesce(False)
        r.route_pack_submit(0, b"a.b:x|c\nc.d:2|c\n")
        assert len(r.route_pack_result(0)[0]) == 2


def test_logs_trace_and_statistics_are_those_of_the_switch_off(pkg):
    """The log text at TRACE level, the trace and the name statistics, byte for byte, with the switch off and on."""
    n = 5
    outs = []
    for on in (False, True):
        with pkg.Router(n, 1 << 17) as r:
            r.set_logtext(pkg.SR_LOG_TRACE)
            r.set_name_stats(True, hll_p=6, cms_rows=3, cms_width=256, hot_slots=16, hot_div=8, hot_min_lines=2)
            r.set_trace(True)
            if on:
                r.set_validate(pkg.ValidateConfig(E.DROP_ALL))
            got = []
            for b in range(3):
                r.route_pack_set_prefix(b % 2, b"T%d " % b, b"W%d " % b)
                r.route_pack_submit(b % 2, traffic(70 + b, 1200), [0] * n if b == 0 else None)
                r.route_pack_result(b % 2)
                got.append((r.route_pack_logtext(b % 2), r.route_pack_trace(b % 2)))
            if on:
                assert int(r.route_pack_validate(0)[1]) > 100
            outs.append((got, r.stats_read()))
    for (la, ta), (lb, tb) in zip(outs[0][0], outs[1][0]):
        assert la[0] == lb[0] and la[1] == lb[1] and np.array_equal(la[2], lb[2]) and np.array_equal(la[3], lb[3])
        assert len(la[0]) > 1000
        assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])
    a, b = outs[0][1], outs[1][1]
    assert np.array_equal(a.lines, b.lines) and np.array_equal(a.cells, b.cells) and np.array_equal(a.regs, b.regs)
    assert np.array_equal(a.hot, b.hot) and a.n_hot > 0
