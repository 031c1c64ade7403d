"""GPU: seeded random walks over a live context of the host-memory submit path. A step toggles one or two of the six
switches (replacing a rule set by one of another size, the same set again after None, the stages' close calls,
another log capacity, the statistics off and on), changes the alive bits or the lane layout, submits 0, 1 or 40..3000
hostile lines by one of the three ways (sometimes with the host's fill, sometimes with staged prefixes and datagram
ends) or collects a slot in flight. Every submission is compared, bit for bit, with the model of
tests/switch_model.py, and so are the name statistics and the rule hits the context carries; nothing is skipped,
retried or tolerated."""
from __future__ import annotations

import errno

import numpy as np
import pytest

import stats_expect as S
import switch_model as M
from test_gpu_switch_matrix import _host_arena

pytestmark = pytest.mark.gpu

MAX_BATCH = 1 << 19   # 3000 hostile lines are up to 300 KB
STEPS = 40
# (seed, N, first layout, coalescing on before the first submission)
WALKS = [(1, 6, 0, False), (2, 5, 0, True), (3, 70, 0, False), (4, 7, 3, False), (5, 1100, 1, False)]
LOGS = [(None,), (M.WARN, 0, 0), (M.TRACE, 0, 0), (M.TRACE, 50000, 300), (M.WARN, 1 << 20, 64), (M.TRACE, 3 << 20, 2047)]
STATS_CFG = dict(hll_p=6, cms_rows=3, cms_width=256, hot_slots=16, hot_div=8, hot_min_lines=2)
PREFIXES = (b"T:", b"2026-01-01 00:00:00 [WARN] th3 ")


class Walk:
    def __init__(self, pkg, r, n, seed):
        self.pkg, self.r, self.n = pkg, r, n
        self.m = M.Model(n, MAX_BATCH)
        self.rng = np.random.default_rng([0xA1C, seed])
        self.seed = seed
        self.inflight = {}        # slot -> (expectation, label, what must stay alive until it is collected)
        self.step = 0
        self.busy_checked = False
        self.submitted = 0
        self.log_on = False

    # ---- both sides -------------------------------------------------------------------------------------------
    def both(self, name, *a, **k):
        getattr(self.r, name)(*a, **k)
        getattr(self.m, name)(*a, **k)

    def set_rules(self, rules):
        self.r.set_name_rules(self.pkg.RuleSet(rules) if rules is not None else None)
        self.m.set_name_rules(rules)

    def set_log(self, args):
        self.both("set_logtext", *args)
        self.log_on = args[0] is not None

    def collect(self, slot):
        x, label, _keep = self.inflight.pop(slot)
        M.check(self.r, slot, x, label)

    def drain(self):
        for slot in sorted(self.inflight):
            self.collect(slot)

    def check_carried(self, label):
        self.drain()
        if self.m.stats is not None:
            assert S.same(self.r.stats_read(), self.m.stats.read()) == [], f"{label}: name statistics"
        if self.m.hits is not None:
            assert self.r.rules_read().tolist() == self.m.hits.tolist(), f"{label}: rule hits"

    # ---- the steps --------------------------------------------------------------------------------------------
    def toggle(self, label):
        """One switch changes (the walk has drained). Returns what it did."""
        rng, m = self.rng, self.m
        k = int(rng.integers(0, 11))
        if k == 0:
            self.set_rules(M.RULES if m.rules != M.RULES else M.RULES_B)       # a set of another size replaces it
            return "rules: another set"
        if k == 1:
            self.set_rules(None)
            return "rules off"
        if k == 2:
            self.rules_off_and_same_again(label)
            return "rules: None, the same set again"
        if k == 3:
            self.both("rules_close")
            return "rules_close"
        if k == 4:
            self.both("set_coalesce", not m.co_on, [0, 16, 1024][int(rng.integers(0, 3))])
            return f"coalesce {m.co_on}"
        if k == 5:
            self.both("coalesce_close")
            return "coalesce_close"
        if k == 6:
            self.both("set_payloads", not m.payloads)
            return f"payloads {m.payloads}"
        if k == 7:
            self.both("set_trace", not m.trace)
            return f"trace {m.trace}"
        if k in (8, 9):
            args = LOGS[int(rng.integers(0, len(LOGS)))]
            self.set_log(args)
            return f"logtext {args}"
        self.stats_off_and_on(label) if m.stats_on else self.both("set_name_stats", True, **STATS_CFG)
        return "stats"

    def rules_off_and_same_again(self, label):
        """set_name_rules(None), then the same set: a new stage, whose hits restart from zero."""
        rules = self.m.rules_open or M.RULES
        self.set_rules(None)
        self.set_rules(rules)
        assert self.r.rules_read().tolist() == [[0, 0]] * (len(rules) + 1), f"{label}: the hits did not restart"

    def stats_off_and_on(self, label):
        """set_name_stats(False), a submission that is not counted, then True: the statistics continue."""
        before = self.m.stats.read()
        self.both("set_name_stats", False)
        self.submit(label + ": with the statistics off", way="sync")
        self.both("set_name_stats", True, hll_p=4)   # the open stage keeps its configuration
        assert S.same(self.r.stats_read(), before) == [], f"{label}: the statistics did not continue"

    def alive(self):
        u = self.rng.random()
        a = [1] * self.n if u < 0.2 else [0] * self.n if u < 0.27 else (self.rng.random(self.n) > 0.25).astype(int).tolist()
        self.both("set_alive", a)

    def busy_check(self, label, slot):
        """Every switch whose change needs an idle context answers -EBUSY while a slot is in flight, and nothing
        changes."""
        r, pkg = self.r, self.pkg
        calls = {
            "set_name_rules": lambda: r.set_name_rules(pkg.RuleSet(M.RULES_B)),
            "set_name_rules(None)": lambda: r.set_name_rules(None),
            "rules_close": r.rules_close,
            "set_coalesce": lambda: r.set_coalesce(True),
            "set_coalesce(False)": lambda: r.set_coalesce(False),
            "coalesce_close": r.coalesce_close,
            "set_logtext": lambda: r.set_logtext(M.TRACE),
            "set_logtext(None)": lambda: r.set_logtext(None),
            "set_name_stats": lambda: r.set_name_stats(True),
            "set_name_stats(False)": lambda: r.set_name_stats(False),
        }
        for what, call in calls.items():
            with pytest.raises(pkg.SrError) as ei:
                call()
            assert ei.value.errno == errno.EBUSY, f"{label}: {what} with a slot in flight"
        # sr_set_trace and sr_set_payloads promise no -EBUSY (include/sr_route.h): they hold for later submissions,
        # and the slot in flight keeps what it was submitted with, which its collection checks
        r.set_trace(not self.m.trace)
        r.set_payloads(not self.m.payloads)
        self.collect(slot)
        r.set_trace(self.m.trace)
        r.set_payloads(self.m.payloads)
        self.busy_checked = True

    def submit(self, label, way=None, count=None):
        rng, r, m, n = self.rng, self.r, self.m, self.n
        way = way or ("submit", "slots", "sync")[int(rng.integers(0, 3))]
        if count is None:
            u = rng.random()
            count = 0 if u < 0.1 else 1 if u < 0.2 else int(40 * 75 ** rng.random())   # 40..3000, mostly small
        data = M.hostile_traffic(1000 * self.seed + self.step * 8 + self.submitted % 8, count)
        self.submitted += 1
        assert len(data) <= MAX_BATCH
        fill = rng.integers(0, 1451, n).tolist() if rng.random() < 0.25 else None
        staged = self.log_on and rng.random() < 0.5
        dgrams = M.datagrams(data, self.submitted)
        label = f"{label}: {way} of {count} lines"
        if way == "sync":
            if count == 0:
                return   # sr_route_pack_batch of nothing submits nothing
            fill = list(m.fills) if fill is None else fill   # the call always brings the host's fill
            ends = M.ends_of(dgrams) if staged else None
            pf = PREFIXES if staged else (b"", b"")
            if staged:
                r.route_pack_set_prefix(2, *pf)
                r.route_pack_set_ends(2, ends)
            got = r.route_pack(data, fill)
            M.check(r, 2, m.submit(2, data, fill, ends, pf), label, result=got)
            return
        slot = int(rng.integers(0, 2))
        if slot in self.inflight:
            self.collect(slot)
        pf = PREFIXES if staged else (b"", b"")
        if staged:
            r.route_pack_set_prefix(slot, *pf)
        if way == "slots":
            buf, lens = _host_arena(self.pkg, dgrams)
            r.route_pack_submit_slots(slot, buf, 4096, lens, fill)
            self.inflight[slot] = (m.submit_slots(slot, dgrams, fill, pf), label, buf)
        else:
            ends = M.ends_of(dgrams) if staged else None
            if staged:
                r.route_pack_set_ends(slot, ends)
            r.route_pack_submit(slot, data, fill)
            self.inflight[slot] = (m.submit(slot, data, fill, ends, pf), label, data)
        if not self.busy_checked:
            self.busy_check(label, slot)

    def random_step(self, label):
        u = self.rng.random()
        if u < 0.33:
            self.drain()
            what = self.toggle(label)
            if self.rng.random() < 0.3:
                what += ", " + self.toggle(label)
            return what
        if u < 0.41:
            self.alive()
            return "alive"
        if u < 0.46:
            self.r.set_layout(int(self.rng.integers(0, 4)))
            return "layout"
        if u < 0.93 or not self.inflight:
            self.submit(label)
            return "submission"
        self.collect(sorted(self.inflight)[int(self.rng.integers(0, len(self.inflight)))])
        return "collect"


@pytest.mark.parametrize("seed,n,layout,coalesce_first", WALKS, ids=[f"walk{w[0]}-N{w[1]}" for w in WALKS])
def test_walk(pkg, seed, n, layout, coalesce_first):
    with pkg.Router(n, MAX_BATCH) as r:
        r.set_layout(layout)
        w = Walk(pkg, r, n, seed)
        if coalesce_first:
            w.both("set_coalesce", True, 16)      # on before the context has routed anything
        else:                                      # the original input buffer gets a history first
            w.both("set_trace", True)
            w.both("set_name_stats", True, **STATS_CFG)
            w.set_rules(M.RULES)
            for k, way in enumerate(("submit", "slots", "sync", "submit", "submit")):
                w.step = -5 + k
                w.submit(f"before coalescing #{k}", way=way, count=[300, 700, 40, 0, 1500][k])
            w.drain()
            w.both("set_coalesce", True)           # the input buffer is allocated again, with the text's room
        done = set()
        for step in range(STEPS):
            w.step = step
            label = f"walk {seed} step {step}"
            if step == 12:                         # what every walk does at least once, whatever it draws
                w.drain()
                w.rules_off_and_same_again(label)
                done.add("rules again")
            elif step == 24:
                w.drain()
                if not w.m.stats_on:
                    w.both("set_name_stats", True, **STATS_CFG)
                    w.submit(label, way="submit", count=300)
                    w.drain()
                w.stats_off_and_on(label)
                done.add("stats again")
            elif step == 32:
                w.drain()
                w.both("rules_close")
                w.both("coalesce_close")
                w.submit(label + ": after the close calls", way="submit", count=300)
                w.drain()
                w.set_rules(M.RULES_B)
                w.both("set_coalesce", True, 16)
            else:
                done.add(w.random_step(label).split(":")[0].split(",")[0].split(" ")[0])
            if step % 8 == 7:
                w.check_carried(label)
        w.check_carried(f"walk {seed} end")
        assert w.busy_checked and w.submitted > 10 and {"rules again", "stats again", "submission"} <= done
