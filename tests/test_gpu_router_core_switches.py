"""GPU: the router data thread with every combination of sr_core_set_name_rules, sr_core_set_coalesce,
sr_core_set_payloads, sr_core_set_device_log and sr_core_set_name_stats, through sr_core_route, sr_core_submit and
sr_core_submit_slots, on a session of the hostile traffic of tests/switch_model.py. The pattern of
tests/test_gpu_router_core_rules.py: the kept and merged lines of a batch, in order, are themselves a framed batch, so
the packets, the final state and the counters are those of a core with every switch off that is fed these batches
instead, and the logs are those of a core with every switch off that is fed the originals. The stages' totals
(sr_core_coalesce_counts, sr_core_name_rule_hits) are the restatements', the name statistics those of a core with
no other switch on, and with the device log on the batches' messages do come from the device's text."""
from __future__ import annotations

import importlib

import numpy as np
import pytest

import coalesce_expect as CE
import rules_expect as E
import stats_expect as S
import switch_model as M

pytestmark = pytest.mark.gpu

N = 5
MODES = [(7, "copy"), (7, "async"), (7, "slots")]
STATS_CFG = dict(hll_p=6, cms_rows=3, cms_width=256, hot_slots=16, hot_div=8, hot_min_lines=2)
_REFS = {}   # the switch-off replays, by what they depend on


def session(log_level=3):
    """The hostile lines as datagrams of at most 4095 bytes, with the alive toggles, flush and ping ticks of the
    other core tests' sessions."""
    dgrams = M.datagrams(M.hostile_traffic(41, 1500), 41)
    assert 60 < len(dgrams) and max(len(d) for d in dgrams) <= 4095
    events = [("alive", [1] * N)]
    for g, d in enumerate(dgrams):
        events.append(("dgram", d))
        if g == 20:
            events.append(("alive", [1, 0, 1, 1, 0]))
        if g == 33:
            events.append(("flush",))
        if g == 41:
            events += [("ping",), ("alive", [1] * N)]
    return {"n": N, "ds_hosts": ["h%d" % i for i in range(N)], "ds_data_ports": [str(9000 + i) for i in range(N)],
            "ping_prefix": "statsd-router.ping", "hostname": "host", "data_port": 8125, "log_level": log_level,
            "events": events}


def _replay(pkg, oracle, f, group, mode, *, rules=False, coalesce=False, payloads=False, device_log=False,
            stats=False, rewrite=None, reverse=False):
    """The session through a core with the given switches. rewrite = (rules, coalesce): every batch is replaced by
    the lines the restatements keep and merge. reverse: the switches are set in the opposite order."""
    core_mod = importlib.import_module("statsd-router_amd.core")
    core = core_mod.Core(f["n"], f["ds_hosts"], f["ds_data_ports"], f["ping_prefix"], f["hostname"], f["data_port"],
                         max_batch_bytes=1 << 18, log_level=f["log_level"])
    setters = [(payloads, lambda: core.set_payloads(True)), (device_log, lambda: core.set_device_log(True)),
               (stats, lambda: core.set_name_stats(True, **STATS_CFG)),
               (rules, lambda: core.set_name_rules(pkg.RuleSet(M.RULES))), (coalesce, lambda: core.set_coalesce(True))]
    for on, call in (setters[::-1] if reverse else setters):
        if on:
            call()
    alive = [0] * f["n"]
    pend = []
    hits = np.zeros((len(M.RULES) + 1, 2), np.uint64)
    merged = [0, 0, 0, 0]

    def rewritten(framed):
        recs, hashes, cnt = oracle.route(framed, f["n"], alive)
        out, out_hashes, whole = recs[:cnt], hashes[:cnt], framed
        if rewrite[0]:
            res = E.apply(framed, out, out_hashes, f["n"], M.RULES)
            hits[:] += res.hits
            out, out_hashes = res.out, res.hashes_out
        if rewrite[1]:
            co = CE.coalesce(framed, out, out_hashes, f["n"], CE.DEFAULT_SLOTS, len(framed))
            for q in range(4):
                merged[q] += int(co.counts[q])
            out, whole = co.out, framed + co.text
        return b"".join(whole[int(r["offset"]): int(r["offset"]) + int(r["length"])] for r in out)

    def flush_batch():
        if not pend:
            return
        framed = pkg.frame_datagrams(pend)
        if rewrite is not None:
            {"copy": core.route, "async": core.submit, "slots": core.route}[mode](rewritten(framed) if framed else framed)
        elif mode == "slots":
            core.submit_slots(pend)
        else:
            sizes = [len(pkg.frame_datagrams([d])) for d in pend]
            ends = [int(x) for x, k in zip(np.cumsum(sizes), sizes) if k]   # empty datagrams have no entry
            {"copy": core.route, "async": core.submit}[mode](framed, ends)
        pend.clear()

    for e in f["events"]:
        if e[0] == "dgram":
            pend.append(e[1])
            if len(pend) >= group:
                flush_batch()
            continue
        flush_batch()
        if e[0] == "alive":
            core.set_alive(e[1])
            alive = list(e[1])
        elif e[0] == "flush":
            core.flush_timer()
        elif e[0] == "ping":
            core.ping()
    flush_batch()
    core.drain()
    core.final = {s: core.state(s) for s in range(f["n"])}
    core.co_counts = core.coalesce_counts()
    core.rule_hits = core.name_rule_hits() if rules else None
    core.snapshot = core.name_stats() if stats else None
    core.log_stats = core.device_log_stats()
    core.want_hits, core.want_merged = hits, merged
    core.close()
    return core


def _ref(pkg, oracle, level, group, mode, what, **kw):
    """A replay with no switch on but those of kw, once per session and mode."""
    key = (level, group, mode, what)
    if key not in _REFS:
        _REFS[key] = _replay(pkg, oracle, session(level), group, mode, **kw)
    return _REFS[key]


def _packets(core):
    return {k: v for k, v in core.packets.items() if v}


def _check(pkg, oracle, level, group, mode, rules, coalesce, payloads, device_log, stats, reverse):
    f = session(level)
    label = f"{mode} rules={rules} coalesce={coalesce} payloads={payloads} device_log={device_log} stats={stats}"
    on = _replay(pkg, oracle, f, group, mode, rules=rules, coalesce=coalesce, payloads=payloads, device_log=device_log,
                 stats=stats, reverse=reverse)
    want = _ref(pkg, oracle, level, group, mode, ("rewrite", rules, coalesce), rewrite=(rules, coalesce))
    off = _ref(pkg, oracle, level, group, mode, "off")
    assert _packets(on) == _packets(want), f"{label}: packets"
    assert on.final == want.final, f"{label}: final state"
    if level == 0:   # the ping's own TRACE lines carry the counters, which count the kept and merged lines
        ping = f["ping_prefix"].encode()
        assert [m for m in on.logs if ping not in m[1]] == [m for m in off.logs if ping not in m[1]], f"{label}: logs"
        assert [m for m in on.logs if ping in m[1]] == [m for m in want.logs if ping in m[1]] != [], f"{label}: ping"
        assert len(on.logs) > 1000
    else:
        assert on.logs == off.logs, f"{label}: logs"
    assert on.co_counts == (want.want_merged if coalesce else [0, 0, 0, 0]), f"{label}: coalesce counts"
    if rules:
        assert on.rule_hits.tolist() == want.want_hits.tolist(), f"{label}: rule hits"
    if stats:
        ref = _ref(pkg, oracle, level, group, mode, "stats", stats=True)
        assert S.same(on.snapshot, ref.snapshot) == [], f"{label}: name statistics"
    if device_log:
        assert on.log_stats[0] > 0, f"{label}: no batch's log came from the device"
    return want


@pytest.mark.parametrize("coalesce", [False, True], ids=["no-coalesce", "coalesce"])
@pytest.mark.parametrize("rules", [False, True], ids=["no-rules", "rules"])
@pytest.mark.parametrize("group,mode", MODES)
def test_session_under_every_combination(pkg, oracle, group, mode, rules, coalesce):
    """Log level 3: the eight combinations of payloads, device log and name statistics under one setting of the
    rules and the coalescing (that is 32 combinations a mode)."""
    k = 0
    for payloads in (False, True):
        for device_log in (False, True):
            for stats in (False, True):
                want = _check(pkg, oracle, 3, group, mode, rules, coalesce, payloads, device_log, stats, reverse=k % 2 == 1)
                k += 1
    if rules:
        assert int(want.want_hits[:-1, 0].sum()) > 0
    if coalesce:
        assert want.want_merged[2] > 0
    ref = _ref(pkg, oracle, 3, group, mode, "stats", stats=True)
    assert ref.snapshot.n_hot > 0 and len(_ref(pkg, oracle, 3, group, mode, "off").logs) > 0


@pytest.mark.parametrize("coalesce", [False, True], ids=["no-coalesce", "coalesce"])
@pytest.mark.parametrize("rules", [False, True], ids=["no-rules", "rules"])
@pytest.mark.parametrize("group,mode", MODES)
def test_session_at_trace_level(pkg, oracle, group, mode, rules, coalesce):
    """Log level 0 with the payloads and the device log on: the device formats every line's hash and pick from the
    original input-order records, on hostile bytes, as the host formatter of the switch-off core does."""
    for stats in (False, True):
        _check(pkg, oracle, 0, group, mode, rules, coalesce, True, True, stats, reverse=stats)
