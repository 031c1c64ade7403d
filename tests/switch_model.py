"""One model of a context of the host-memory submit path (pack_submit in csrc/sr_route.hip) with its six switches,
composed from the restatements the suite already has: the oracle's routing and packing, tests/rules_expect.py,
tests/coalesce_expect.py, tests/payload_expect.py, tests/log_expect.py and tests/stats_expect.py. A plain helper
module (no fixtures, no test, no GPU): `hostile_traffic` is the batch the switch tests submit, `Model` says what
every getter of a slot must return after a submission, `check` compares a live context with it, bit for bit.
tests/test_switch_model.py checks on the CPU that the traffic really exercises the stages."""
from __future__ import annotations

import errno

import numpy as np

import byte_streams
import coalesce_expect as CE
import log_expect as L
import payload_expect as X
import rules_expect as E
import sr_oracle as oracle
import stats_expect as S
from rules_expect import DROP, EXACT, KEEP, PREFIX

RULES = [(b"debug.", PREFIX, DROP), (b"debug.keep.", PREFIX, KEEP), (b"svc.req.7", EXACT, DROP),
         (b"host.hot", EXACT, DROP), (b"\x00\xff", PREFIX, DROP)]
# a second set of another size, for the tests that replace a set on a live context
RULES_B = [(b"svc.", PREFIX, DROP), (b"svc.lat.", PREFIX, KEEP), (b"n", PREFIX, DROP)]
LONG_NAMES = (1, 64, 65, 700, 1424, 1425)   # name lengths of the long-name lines, up to coalescing's limit
OFF, WARN, TRACE = None, L.WARN, L.TRACE
MATRIX_SEED = 7   # the 300-line batch of the switch matrix: 23 KB, two route tiles


def hostile_lines(seed, count):
    """The lines (without '\\n') of hostile_traffic."""
    rng = np.random.default_rng([0x5317C4, seed])
    lines = []
    for u, k, v in zip(rng.random(count), rng.integers(0, 12, count).tolist(), rng.integers(-500, 500, count).tolist()):
        if u < 0.15:
            lines.append(b"host.hot:1|c")
        elif u < 0.30:
            lines.append(b"debug.t%d:%d|c" % (k, v))
        elif u < 0.40:
            lines.append(b"debug.keep.t%d:1|c" % k)
        elif u < 0.65:
            lines.append(b"svc.req.%d:%d|c" % (k, v))
        elif u < 0.72:
            lines.append(b"svc.lat.%d:%d|ms" % (k, v))
        elif u < 0.76:
            lines.append(b"bad")
        elif u < 0.80:
            lines.append(b"debug.no colon in this line")
        elif u < 0.85:   # a dropped prefix of bytes that are no text
            lines.append(b"\x00\xff" + byte_streams.uniform_name(rng, int(rng.integers(1, 40))) + b":%d|c" % v)
        elif u < 0.90:   # arbitrary bytes, repeating
            lines.append(byte_streams.uniform_name(np.random.default_rng([seed, k]), k + 1) * 3 + b":%d|c" % v)
        elif u < 0.93:
            lines.append(byte_streams._valid_line(rng, int(rng.integers(6, 1450)))[:-1])
        elif u < 0.95:   # no colon, too short, 1450 and 1451 bytes
            lines.append(byte_streams._invalid_line(rng)[:-1])
        elif u < 0.98:
            lines.append(b"n" * LONG_NAMES[k % len(LONG_NAMES)] + b":%d|c" % v)
        else:            # negative sums, high bytes
            lines.append(b"x\x80\xfe.%d:-%d|c" % (k % 3, abs(v)))
    return lines


def hostile_traffic(seed, count) -> bytes:
    """A framed batch of `count` lines: names the rules drop and keep, counters that merge (some to a sum <= 0, some
    with names of up to 1425 bytes, some of arbitrary bytes), timers, and lines that are invalid in every way."""
    return b"".join(l + b"\n" for l in hostile_lines(seed, count))


def datagrams(data: bytes, seed, most=40, limit=4095):
    """The lines of a framed batch cut into datagrams of 1..`most` lines and at most `limit` bytes, each without its
    final '\\n' (framing puts it back) unless its last line is empty. Framed again they are `data`."""
    rng = np.random.default_rng([0xD6, seed])
    lines = data.split(b"\n")[:-1] if data else []
    out, i = [], 0
    while i < len(lines):
        k, size = 1, len(lines[i]) + 1
        want = int(rng.integers(1, most + 1))
        while k < want and i + k < len(lines) and size + len(lines[i + k]) + 1 <= limit:
            size += len(lines[i + k]) + 1
            k += 1
        d = b"\n".join(lines[i:i + k])
        out.append(d + b"\n" if (not lines[i + k - 1] or len(d) == 0) else d)
        i += k
    assert b"".join(oracle.frame(d) for d in out) == data and all(len(d) <= limit for d in out)
    return out


def ends_of(dgrams):
    """The framed datagram ends (empty datagrams have no entry)."""
    sizes = [len(oracle.frame(d)) for d in dgrams]
    return np.array([e for e, k in zip(np.cumsum(sizes), sizes) if k], dtype=np.uint32)


class Expectation:
    """What the getters of a slot must return after one submission; None where the switch was off."""

    def __init__(self):
        self.sorted = self.packets = self.fill_out = self.n_valid = self.probed = None
        self.rules_counts = self.co_text = self.co_counts = None
        self.arena = self.offsets = self.rooms = None
        self.trace = self.logtext = None
        self.log_cap = 0
        self.n_in = 0

    def pack(self):
        return (self.sorted, self.packets, self.fill_out, self.n_valid, self.probed)

    @property
    def total(self):
        return int(self.offsets[-1])


class Model:
    """A context of n downstreams: the switches, and what it carries from one submission to the next (the pending
    bytes' chain, the name statistics, the rule hits). `cache` (a dict) may be shared between models: every stage's
    result depends only on its inputs, which are its key."""

    def __init__(self, n, max_batch, cache=None):
        self.n, self.max_batch = n, max_batch
        self.cache = {} if cache is None else cache
        self.alive = [1] * n
        self.fills = [0] * n
        self.rules = None          # the set that is on
        self.rules_open = None     # the set of the open stage (it outlives the switch)
        self.hits = None
        self.co_on, self.co_slots = False, None   # co_slots: of the open stage
        self.payloads = self.trace = False
        self.log = None            # (level, cap, max_msg)
        self.stats_on, self.stats = False, None

    # ---- the setters of pkg.Router ------------------------------------------------------------------------------
    def set_alive(self, alive):
        self.alive = [int(a) for a in alive]

    def set_name_rules(self, rules):
        if rules is None:
            self.rules = None
            return
        assert E.check(rules)
        self.rules = self.rules_open = list(rules)
        self.hits = np.zeros((len(rules) + 1, 2), np.uint64)   # a new set replaces the old one, hits included

    def rules_close(self):
        self.rules = self.rules_open = self.hits = None

    def set_coalesce(self, on=True, slots=0):
        if on and self.co_slots is None:   # the slot count is fixed once the stage is open
            self.co_slots = slots or CE.DEFAULT_SLOTS
        self.co_on = bool(on)

    def coalesce_close(self):
        self.co_on, self.co_slots = False, None

    def set_payloads(self, on=True):
        self.payloads = bool(on)

    def set_trace(self, on=True):
        self.trace = bool(on)

    def set_logtext(self, level, cap=0, max_msg=0):
        self.log = None if level is None else (level, cap or self.max_batch * 8 + 65536, max_msg)

    def set_name_stats(self, on=True, **cfg):
        if on and self.stats is None:      # the configuration is that of the first call
            self.stats = S.Stats(self.n, cfg)
        self.stats_on = bool(on)

    # ---- the stages, each cached by its inputs ------------------------------------------------------------------
    def _memo(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def _route(self, data):
        def make():
            arr = np.frombuffer(data, np.uint8)
            recs, hashes, n_in = oracle.route(arr, self.n, self.alive)
            assert n_in == len(recs)
            return recs, hashes, oracle.probed_dead(arr, self.n, self.alive)
        return self._memo(("route", data, self.n, tuple(self.alive)), make)

    def submit(self, slot, data, fill=None, ends=None, prefixes=(b"", b"")):
        """A framed batch by sr_route_pack_submit (slot 0 or 1) or sr_route_pack_batch (slot 2)."""
        assert slot in (0, 1, 2) and len(data) <= self.max_batch and (not data or data.endswith(b"\n"))
        n, akey = self.n, (self.n, tuple(self.alive))
        fills = [int(f) for f in (fill if fill is not None else self.fills)]
        recs, hashes, probed = self._route(data)
        x = Expectation()
        x.n_in = len(recs)
        out, out_hashes, whole = recs, hashes, data
        rkey = ckey = None
        if self.rules is not None:
            rkey = tuple(self.rules)
            res = self._memo(("rules", data, akey, rkey), lambda: E.apply(data, recs, hashes, n, self.rules))
            x.rules_counts = res.counts
            self.hits += res.hits
            out, out_hashes = res.out, res.hashes_out
        if self.co_on:
            ckey = self.co_slots
            r_in, h_in = out, out_hashes
            co = self._memo(("coalesce", data, akey, rkey, ckey),
                            lambda: CE.coalesce(data, r_in, h_in, n, self.co_slots, len(data)))
            assert co.complete
            x.co_text, x.co_counts = co.text, co.counts
            out, whole = co.out, data + co.text
        pkey = ("pack", data, akey, rkey, ckey, tuple(fills))
        x.sorted, x.packets, x.fill_out, x.n_valid = self._memo(pkey, lambda: oracle.pack_packets(out, n, fills, probed))
        x.probed = probed
        if self.payloads:
            pending = {k: bytes(f) for k, f in enumerate(fills)}
            x.arena, x.offsets, x.rooms = self._memo(("payload",) + pkey[1:],
                                                     lambda: X.flat_expectation(whole, x.sorted, x.packets, pending))
        if self.trace:
            x.trace = (recs, hashes)   # the input's, never the kept ones
        if self.log is not None:
            level, cap, max_msg = self.log
            e = None if (ends is None or level != TRACE) else np.asarray(ends, np.uint32)
            x.logtext = self._memo(("log", data, akey, None if e is None else e.tobytes(), level, tuple(prefixes), max_msg),
                                   lambda: L.expect(data, recs, hashes, e, n, level, prefixes, max_msg))
            x.log_cap = cap
        if self.stats_on and data:
            self.stats.update([(data, recs, hashes)])   # the route's records, whatever the other switches say
        self.fills = [int(f) for f in x.fill_out]
        return x

    def submit_slots(self, slot, dgrams, fill=None, prefixes=(b"", b"")):
        """Datagrams by sr_route_pack_submit_slots: framed on the device, their ends known to the log."""
        assert slot in (0, 1)
        return self.submit(slot, b"".join(oracle.frame(d) for d in dgrams), fill, ends_of(dgrams), prefixes)


def _busy(fn, slot, label):
    try:
        fn(slot)
    except OSError as e:   # pkg.SrError
        assert e.errno == errno.EBUSY, f"{label}: {fn.__name__} with its switch off gave errno {e.errno}"
        return
    raise AssertionError(f"{label}: {fn.__name__} answered although its switch was off at this submission")


def check(r, slot, x, label, result=None):
    """Everything the switches of that submission expose, against expectation x. Slots 0 and 1 are collected here;
    `result` is what route_pack returned (slot 2). A getter whose switch was off must answer -EBUSY: a slot never
    hands out what an earlier submission left in its page-locked memory."""
    from test_gpu_mtu import assert_pack_equal
    from test_gpu_payloads import _check_host

    got = r.route_pack_result(slot) if result is None else result
    try:
        assert_pack_equal(got, x.pack())
    except AssertionError as e:
        raise AssertionError(f"{label}: {e}") from None
    if x.rules_counts is None:
        _busy(r.route_pack_rules, slot, label)
    else:
        assert r.route_pack_rules(slot).tolist() == x.rules_counts.tolist(), f"{label}: rules counts"
    if x.co_counts is None:
        _busy(r.route_pack_coalesced, slot, label)
    else:
        text, counts = r.route_pack_coalesced(slot)
        assert counts.tolist() == x.co_counts.tolist(), f"{label}: coalesce counts {counts.tolist()} != {x.co_counts.tolist()}"
        assert text == x.co_text, f"{label}: merged text"
    if x.offsets is None:
        _busy(r.route_pack_payloads, slot, label)
    else:
        _check_host(r.route_pack_payloads(slot), x, label)
    if x.trace is None:
        _busy(r.route_pack_trace, slot, label)
    else:
        recs, hs = r.route_pack_trace(slot)
        assert np.array_equal(recs, x.trace[0]), f"{label}: trace records"
        assert np.array_equal(hs, x.trace[1]), f"{label}: trace hashes"
    if x.logtext is None:
        _busy(r.route_pack_logtext, slot, label)
    else:
        text, total, offs, lv, ok = r.route_pack_logtext(slot)
        want_text, want_offs, want_lv = x.logtext
        assert total == len(want_text), f"{label}: log total {total} != {len(want_text)}"
        assert ok == (total <= x.log_cap), f"{label}: log complete"
        k = lv.size if not ok else len(want_lv)
        assert text == want_text[:x.log_cap], f"{label}: log text"
        assert np.array_equal(offs, want_offs[:k + 1]) and np.array_equal(lv, want_lv[:k]), f"{label}: log index"
