"""GPU: the router data thread with sr_core_set_name_rules, through sr_core_route, sr_core_submit and
sr_core_submit_slots, with the payloads switch on and off. The kept lines of a batch, in order, are themselves a
framed batch (tests/rules_expect.py gives them), so what the core emits with the switch on is what the same core
emits with the switch off when it is fed those batches instead: every packet per downstream, every pending buffer
and every counter. The log output is that of the same session with the switch off."""
from __future__ import annotations

import importlib

import numpy as np
import pytest

import rules_expect as E
from rules_expect import DROP, EXACT, KEEP, PREFIX

pytestmark = pytest.mark.gpu

RULES = [(b"core.debug.", PREFIX, DROP), (b"core.debug.keep.", PREFIX, KEEP), (b"core.hot", EXACT, DROP),
         (b"no colon", PREFIX, DROP)]


def session(n=5, log_level=3):
    """A scripted session: names that the rules drop and keep, invalid lines; alive toggles, flush and ping ticks
    between the datagrams."""
    rng = np.random.default_rng(12)
    events = [("alive", [1] * n)]
    for g in range(60):
        lines = []
        for u, k, v in zip(rng.random(int(rng.integers(1, 60))), rng.integers(0, 12, 60), rng.integers(0, 900, 60)):
            if u < 0.25:
                lines.append(b"core.hot:1|c")
            elif u < 0.45:
                lines.append(b"core.debug.t%d:%d|c" % (k, v))
            elif u < 0.55:
                lines.append(b"core.debug.keep.t%d:%d|c" % (k, v))
            elif u < 0.8:
                lines.append(b"core.req.%d:%d|c" % (k, v))
            elif u < 0.9:
                lines.append(b"core.hot.%d:%d|ms" % (k, v))
            elif u < 0.95:
                lines.append(b"bad")
            else:
                lines.append(b"no colon in this line")
        events.append(("dgram", b"\n".join(lines) + (b"\n" if g % 2 else b"")))
        if g == 20:
            events.append(("alive", [1, 0, 1, 1, 0][:n]))
        if g == 33:
            events.append(("flush",))
        if g == 41:
            events += [("ping",), ("alive", [1] * n)]
    return {"n": n, "ds_hosts": ["h%d" % i for i in range(n)], "ds_data_ports": [str(9000 + i) for i in range(n)],
            "ping_prefix": "statsd-router.ping", "hostname": "host", "data_port": 8125, "log_level": log_level,
            "events": events}


def _replay(pkg, oracle, f, group, mode, rules, payloads, rewrite=False):
    """The session through a core. rewrite: every batch is replaced by its kept lines (the restatement's)."""
    core_mod = importlib.import_module("statsd-router_amd.core")
    core = core_mod.Core(f["n"], f["ds_hosts"], f["ds_data_ports"], f["ping_prefix"], f["hostname"], f["data_port"],
                         max_batch_bytes=1 << 20, log_level=f["log_level"])
    if payloads:
        core.set_payloads(True)
    if rules:
        core.set_name_rules(pkg.RuleSet(RULES))
    alive = [0] * f["n"]
    pend = []
    hits = np.zeros((len(RULES) + 1, 2), np.uint64)

    def flush_batch():
        if not pend:
            return
        framed = pkg.frame_datagrams(pend)
        if rewrite:
            if framed:
                recs, hashes, cnt = oracle.route(framed, f["n"], alive)
                res = E.apply(framed, recs[:cnt], hashes[:cnt], f["n"], RULES)
                hits[:] += res.hits
                framed = b"".join(framed[int(r["offset"]): int(r["offset"]) + int(r["length"])] for r in res.out)
            {"copy": core.route, "async": core.submit, "slots": core.route}[mode](framed)
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
    final = {s: core.state(s) for s in range(f["n"])}
    got_hits = core.name_rule_hits() if rules else None
    core.close()
    return core, final, got_hits, hits


MODES = [(1, "copy"), (7, "copy"), (1000, "async"), (7, "async"), (1, "slots"), (7, "slots")]


@pytest.mark.parametrize("payloads", [False, True], ids=["lines", "payloads"])
@pytest.mark.parametrize("group,mode", MODES)
def test_session(pkg, oracle, group, mode, payloads):
    f = session()
    on, final_on, got_hits, _ = _replay(pkg, oracle, f, group, mode, True, payloads)
    want, final_want, _, hits = _replay(pkg, oracle, f, group, mode, False, payloads, rewrite=True)
    off, _, _, _ = _replay(pkg, oracle, f, group, mode, False, payloads)
    assert {k: v for k, v in on.packets.items() if v} == {k: v for k, v in want.packets.items() if v}
    assert final_on == final_want
    assert on.logs == off.logs                       # the WARN lines of the original batches, in their order
    assert got_hits.tolist() == hits.tolist()
    assert int(hits[0, 0]) > 50 and int(hits[1, 0]) > 20 and int(hits[2, 0]) > 100 and int(hits[3, 0]) == 0
    sent = b"".join(p for ps in on.packets.values() for p in ps)
    assert b"core.hot:" not in sent and b"core.debug.t" not in sent
    assert b"core.debug.keep.t" in sent and b"core.hot." in sent and b"core.req." in sent


def test_session_at_trace_level(pkg, oracle):
    """TRACE: every line's hash and pick is logged from the original input-order records. The ping's own lines
    carry the traffic and packet counters, which count the kept lines: they are compared with the rewritten
    session's, everything else with the switch-off session's."""
    f = session(log_level=0)
    ping = f["ping_prefix"].encode()
    for group, mode in [(7, "copy"), (7, "async"), (7, "slots")]:
        on, final_on, _, _ = _replay(pkg, oracle, f, group, mode, True, True)
        off, _, _, _ = _replay(pkg, oracle, f, group, mode, False, True)
        want, final_want, _, _ = _replay(pkg, oracle, f, group, mode, False, True, rewrite=True)
        data = lambda logs: [m for m in logs if ping not in m[1]]
        assert data(on.logs) == data(off.logs) and len(on.logs) > 1000
        assert [m for m in on.logs if ping in m[1]] == [m for m in want.logs if ping in m[1]] != []
        assert {k: v for k, v in on.packets.items() if v} == {k: v for k, v in want.packets.items() if v}
        assert final_on == final_want


def test_switch_needs_an_idle_core_hits_reset_and_pings_are_exempt(pkg):
    core_mod = importlib.import_module("statsd-router_amd.core")
    with core_mod.Core(2, ["a", "b"], ["1", "2"], "p", "h", 9000, max_batch_bytes=1 << 16) as core:
        core.set_alive([1, 1])
        with pytest.raises(pkg.SrError) as ei:
            core.name_rule_hits()
        assert ei.value.errno == 22   # EINVAL: the switch was never on
        core.submit(b"k:1|c\n" * 10)
        with pytest.raises(pkg.SrError) as ei:
            core.set_name_rules(pkg.RuleSet([(b"k", EXACT, DROP)]))
        assert ei.value.errno == 16   # EBUSY: a batch is in flight
        core.drain()
        core.set_name_rules(pkg.RuleSet([(b"k", EXACT, DROP), (b"p", PREFIX, DROP)]))   # "p" is the ping prefix
        core.submit(b"k:1|c\n" * 400 + b"j:1|c\n" * 3)
        core.ping()                    # drains; its own lines are not subject to the rules
        assert core.name_rule_hits(reset=True).tolist() == [[400, 2400], [0, 0], [3, 18]]
        assert core.name_rule_hits().tolist() == [[0, 0], [0, 0], [0, 0]]
        core.set_name_rules(None)
        core.route(b"k:1|c\n" * 50)
        core.flush_timer()
        sent = b"".join(p for ps in core.packets.values() for p in ps)
        assert sent.count(b"k:1|c\n") == 60 and sent.count(b"j:1|c\n") == 3
        assert any(l.startswith(b"p") for l in sent.split(b"\n"))   # the ping's lines went out under a DROP "p*"
