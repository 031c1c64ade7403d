"""GPU: every combination of the six switches of the host-memory submit path (sr_set_name_rules, sr_set_coalesce,
sr_set_payloads, sr_set_trace, sr_set_name_stats, sr_set_logtext off / WARN / TRACE) on one live context per lane
layout and shard state, in Gray-code order, so that successive combinations differ in one switch and every switch
goes on and off many times. Each combination submits the hostile batch of tests/switch_model.py in the three ways
(double-buffered, as datagram slots, synchronously) and every getter is compared, bit for bit, with the model;
a getter whose switch was off must answer -EBUSY. tests/test_switch_model.py shows on the CPU that the batch has
lines that are dropped, groups that merge and slots that collide: nothing here asserts such counts."""
from __future__ import annotations

import numpy as np
import pytest

import frame_slots as F
import stats_expect as S
import switch_model as M

pytestmark = pytest.mark.gpu

MAX_BATCH = 1 << 17
LAYOUTS = [("uniform", 1), ("segments", 2), ("chunks", 3), ("auto", 0)]


def _alive(n, dead):
    a = [1] * n
    for k in dead:
        a[k] = 0
    return a


# (N, the dead shards): all alive, one shard, the first dead, two dead, more than 64 shards, more than 1024 (where the
# probed-dead replay wants the route's hashes) with a dead shard past the 1024th, every shard dead
STATES = [(6, ()), (1, ()), (7, (0,)), (5, (1, 3)), (100, tuple(range(3, 99, 6))), (1100, (3, 1027)), (3, (0, 1, 2))]
STATE_IDS = ["6", "1", "7-first-dead", "5-two-dead", "100-16-dead", "1100-two-dead", "3-all-dead"]
LOG_ARGS = {M.WARN: (M.WARN, 0, 0), M.TRACE: (M.TRACE, 0, 2047)}   # TRACE cuts the "got packet" messages
PREFIXES = (b"2026-01-01 00:00:00 [TRACE] th0 ", b"W> ")
NAMES = ("rules", "coalesce", "payloads", "trace", "stats")
CACHE = {}   # the model's stages by their inputs: shared by the 96 combinations and the four layouts of a state


def combinations():
    """The 2^5 x 3 combinations as ({switch: on}, log level), each differing from the one before in one switch: the
    reflected Gray code of five bits, walked forwards, backwards and forwards again under the three log levels. The
    third walk starts from "all off" and gives the bits to other switches, so that the switches of the slow bits
    change often too (tests/test_switch_model.py checks the order on the CPU)."""
    gray = [i ^ (i >> 1) for i in range(32)]
    out = []
    for j, level in enumerate((M.OFF, M.WARN, M.TRACE)):
        for g in (gray if j % 2 == 0 else gray[::-1]):
            out.append(({NAMES[(b + (2 if j == 2 else 0)) % 5]: bool(g >> b & 1) for b in range(5)}, level))
    return out


class Pair:
    """A context and its model, switched together."""

    def __init__(self, pkg, r, n, slots, max_batch=MAX_BATCH, cache=None):
        self.pkg, self.r, self.m, self.slots = pkg, r, M.Model(n, max_batch, CACHE if cache is None else cache), slots
        self.state = ({k: False for k in NAMES}, M.OFF)
        self.stats_cfg = dict(hll_p=6, cms_rows=3, cms_width=256, hot_slots=16, hot_div=8, hot_min_lines=2)

    def both(self, name, *a, **k):
        getattr(self.r, name)(*a, **k)
        getattr(self.m, name)(*a, **k)

    def switch(self, on, level):
        """Only what differs from the current state is set: a rule set that is set again would restart its hits."""
        cur, cur_level = self.state
        if on["rules"] != cur["rules"]:
            self.r.set_name_rules(self.pkg.RuleSet(M.RULES) if on["rules"] else None)
            self.m.set_name_rules(M.RULES if on["rules"] else None)
        if on["coalesce"] != cur["coalesce"]:
            self.both("set_coalesce", on["coalesce"], self.slots)
        if on["payloads"] != cur["payloads"]:
            self.both("set_payloads", on["payloads"])
        if on["trace"] != cur["trace"]:
            self.both("set_trace", on["trace"])
        if on["stats"] != cur["stats"]:
            self.both("set_name_stats", on["stats"], **self.stats_cfg)
        if level != cur_level:
            self.both("set_logtext", *(LOG_ARGS[level] if level is not M.OFF else (None,)))
        self.state = (dict(on), level)

    def stage(self, slot, ends=None):
        """The log's prefixes (and datagram ends) of the slot's next submission; () when the log is off."""
        if self.state[1] is M.OFF:
            return (b"", b"")
        self.r.route_pack_set_prefix(slot, *PREFIXES)
        if ends is not None:
            self.r.route_pack_set_ends(slot, ends)
        return PREFIXES

    def check_carried(self, label):
        on, _ = self.state
        if on["stats"]:
            assert S.same(self.r.stats_read(), self.m.stats.read()) == [], f"{label}: name statistics"
        if on["rules"]:
            assert self.r.rules_read().tolist() == self.m.hits.tolist(), f"{label}: rule hits"


def _host_arena(pkg, dgrams):
    arena, lens = F.build_arena(dgrams, 4096)
    buf = pkg.HostBuffer(max(arena.size, 1))
    buf.array[:arena.size] = arena
    return buf, lens


def run_combination(p, i, on, level, data, dgrams, ends, buf, lens, one, fill0, label, data2):
    """The three ways to submit under one combination; slots 0 and 1 are both in flight before either is collected.
    The synchronous call brings another batch (data2), so that what one submission leaves in the context's device
    buffers is never what the next one should find there."""
    r, m = p.r, p.m
    p.switch(on, level)
    a, b = i % 2, 1 - i % 2
    pf = p.stage(a, ends)
    r.route_pack_submit(a, data, fill0)                           # double-buffered, the host's fill, staged ends
    xa = m.submit(a, data, fill0, ends, pf)
    pf = p.stage(b)
    r.route_pack_submit_slots(b, buf, 4096, lens, None)           # datagram slots, chained on the device
    xb = m.submit_slots(b, dgrams, None, pf)
    M.check(r, a, xa, f"{label}: submit")
    M.check(r, b, xb, f"{label}: submit_slots")
    pf = p.stage(2)
    fill = list(m.fills)
    got = r.route_pack(data2, fill)                               # synchronous, slot 2
    M.check(r, 2, m.submit(2, data2, fill, None, pf), f"{label}: route_pack", result=got)
    if i % 8 == 0:
        r.route_pack_submit(a, b"")                               # an empty batch, then one line as one datagram
        xa = m.submit(a, b"")
        obuf, olens = one
        r.route_pack_submit_slots(b, obuf, 4096, olens, None)
        xb = m.submit_slots(b, [b"svc.req.1:5|c"])
        M.check(r, a, xa, f"{label}: empty batch")
        M.check(r, b, xb, f"{label}: one line")
    p.check_carried(label)


@pytest.mark.parametrize("state", range(len(STATES)), ids=STATE_IDS)
@pytest.mark.parametrize("layout", range(len(LAYOUTS)), ids=[l for l, _ in LAYOUTS])
def test_every_combination_on_one_context(pkg, layout, state):
    n, dead = STATES[state]
    alive = _alive(n, dead)
    data = M.hostile_traffic(M.MATRIX_SEED, 300)
    data2 = M.hostile_traffic(M.MATRIX_SEED + 2, 300)
    dgrams = M.datagrams(data, M.MATRIX_SEED)
    ends = M.ends_of(dgrams)
    fill0 = np.random.default_rng(n).integers(0, 1451, n).tolist()
    fill0[0], fill0[-1] = 1449, 1450
    slots = 16 if (layout + state) % 2 else 0                     # the table's size is fixed once the stage is open
    buf, lens = _host_arena(pkg, dgrams)
    one = _host_arena(pkg, [b"svc.req.1:5|c"])
    with pkg.Router(n, MAX_BATCH) as r:
        r.set_layout(LAYOUTS[layout][1])
        p = Pair(pkg, r, n, slots)
        p.both("set_alive", alive)
        for i, (on, level) in enumerate(combinations()):
            label = f"#{i} " + "+".join([k for k in NAMES if on[k]] + ["log%s" % level] * (level is not M.OFF))
            run_combination(p, i, on, level, data, dgrams, ends, buf, lens, one, fill0, label, data2)
        if n > len(dead):
            assert int(p.m.hits[:, 0].sum()) > 0 and p.m.stats.read().total > 0
    buf.close()
    one[0].close()
