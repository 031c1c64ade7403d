"""GPU: the router data thread with sr_core_set_validate, through sr_core_route, sr_core_submit and
sr_core_submit_slots, with the payloads switch on and off. The kept lines of a batch, in order, are themselves a
framed batch (tests/validate_expect.py gives them), so what the core emits with the switch on is what the same core
emits with the switch off when it is fed those batches instead: every packet per downstream, every pending buffer
and every counter. The log output is that of the same session with the switch off."""
from __future__ import annotations

import importlib

import numpy as np
import pytest

import validate_expect as E

pytestmark = pytest.mark.gpu

DROP = E.DROP_ALL & ~(1 << E.TAGS)      # TAGS is counted and kept
KINDS = [b"core.req.%d:%d|c", b"core.lat.%d:%d|ms|@0.5", b"core.g.%d:+%d|g|#env:p", b"core.set.%d:u%d|s", b"core.bad.%d:x%d|c",
         b"core.q.%d:%d|q", b"core.nt.%d:%d", b"core.rate.%d:%d|g|@1", b"core.tag.%d:%d|c|#", b"core.sec.%d:%d|c|x",
         b"core name.%d:%d|c", b"bad", b"no colon in this line"]


def session(n=5, log_level=3):
    """A scripted session: lines of every reason and invalid lines; alive toggles, flush and ping ticks between the
    datagrams."""
    rng = np.random.default_rng(12)
    events = [("alive", [1] * n)]
    for g in range(60):
        m = int(rng.integers(1, 60))
        lines = []
        for q, k, v in zip(rng.integers(0, 2 * len(KINDS), m), rng.integers(0, 12, m), rng.integers(0, 900, m)):
            f = KINDS[q % len(KINDS)] if q >= len(KINDS) else KINDS[0]     # half the lines are plain counters
            lines.append(f % (k, v) if b"%d" in f else f)
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


def _replay(pkg, oracle, f, group, mode, validate, payloads, rewrite=False):
    """The session through a core. rewrite: every batch is replaced by its kept lines (the restatement's)."""
    core_mod = importlib.import_module("statsd-router_amd.core")
    core = core_mod.Core(f["n"], f["ds_hosts"], f["ds_data_ports"], f["ping_prefix"], f["hostname"], f["data_port"],
                         max_batch_bytes=1 << 20, log_level=f["log_level"])
    if payloads:
        core.set_payloads(True)
    if validate:
        core.set_validate(pkg.ValidateConfig(DROP))
    alive = [0] * f["n"]
    pend = []
    hits = np.zeros((E.REASONS, 2), np.uint64)

    def flush_batch():
        if not pend:
            return
        framed = pkg.frame_datagrams(pend)
        if rewrite:
            if framed:
                recs, hashes, cnt = oracle.route(framed, f["n"], alive)
                res = E.apply(framed, recs[:cnt], hashes[:cnt], f["n"], DROP)
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
    got_hits = core.validate_hits() if validate else None
    core.close()
    return core, final, got_hits, hits


MODES = [(1, "copy"), (7, "async"), (1000, "async"), (7, "slots")]


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
    assert (hits[[E.OK, E.NAME_BYTE, E.NO_TYPE, E.TYPE, E.VALUE, E.SECTION, E.RATE, E.TAGS], 0] > 20).all()
    sent = b"".join(p for ps in on.packets.values() for p in ps)
    for gone in (b"core.bad.", b"core.q.", b"core.nt.", b"core.rate.", b"core.sec.", b"core name."):
        assert gone not in sent, gone
    for kept in (b"core.req.", b"core.lat.", b"core.g.", b"core.set.", b"core.tag."):
        assert kept in sent, kept


def test_switch_needs_an_idle_core_hits_reset_and_pings_are_exempt(pkg):
    core_mod = importlib.import_module("statsd-router_amd.core")
    with core_mod.Core(2, ["a", "b"], ["1", "2"], "p", "h", 9000, max_batch_bytes=1 << 16) as core:
        core.set_alive([1, 1])
        with pytest.raises(pkg.SrError) as ei:
            core.validate_hits()
        assert ei.value.errno == 22   # EINVAL: the switch was never on
        core.submit(b"k:1|c\n" * 10)
        with pytest.raises(pkg.SrError) as ei:
            core.set_validate(pkg.ValidateConfig(E.DROP_ALL))
        assert ei.value.errno == 16   # EBUSY: a batch is in flight
        core.drain()
        with pytest.raises(pkg.SrError) as ei:
            core.set_validate(pkg.ValidateConfig(1))
        assert ei.value.errno == 22
        core.set_validate(pkg.ValidateConfig(E.DROP_ALL))
        core.submit(b"k:x|c\n" * 400 + b"j:1|c\n" * 3)
        core.ping()                    # drains; its own lines are not subject and not counted
        want = [[0, 0]] * E.REASONS
        want[E.OK], want[E.VALUE] = [3, 18], [400, 2400]
        assert core.validate_hits(reset=True).tolist() == want
        assert core.validate_hits().tolist() == [[0, 0]] * E.REASONS
        core.set_validate(None)
        core.route(b"k:x|c\n" * 50)
        core.flush_timer()
        sent = b"".join(p for ps in core.packets.values() for p in ps)
        assert sent.count(b"k:x|c\n") == 50 and sent.count(b"j:1|c\n") == 3
        assert any(l.startswith(b"p") for l in sent.split(b"\n"))   # the ping's lines went out
