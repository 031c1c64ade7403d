"""GPU: the router data thread with sr_core_set_sample, through sr_core_route, sr_core_submit and
sr_core_submit_slots, with the payloads switch on and off and with the coalescing on as well (so that a packet's lines
come from all three places: the batch, the sample text and the merged text). The thinned lines of a batch, in order,
are themselves a framed batch (tests/sample_expect.py gives them, batch b under the seed b), so what the core emits
with the switch on is what the same core emits with the switch off when it is fed those batches instead: every packet
per downstream, every pending buffer and every counter. The log output is that of the same session with the switch
off."""
from __future__ import annotations

import importlib

import numpy as np
import pytest

import sample_expect as E

pytestmark = pytest.mark.gpu

LIMIT, TYPES = 4, E.TYPES_ALL
KINDS = [b"core.time:%d%d|ms", b"core.time:%d.%d|ms|#env:p", b"core.hist.%d:%d|h", b"core.req:%d%d|c", b"core.req:%d%d|c",
         b"core.lat.%d:%d|ms|@0.5", b"core.g.%d:+%d|g", b"core.dist:%d%d|d|#a:b,c", b"core.cold.%d:%d|ms", b"core.nt.%d:%d",
         b"bad", b"no colon in this line", b"core.plain.%d:1|c"]


def session(n=5, log_level=3):
    """A scripted session: hot timers, a hot counter, cold names, lines that are not sampleable and invalid lines;
    alive toggles, flush and ping ticks between the datagrams."""
    rng = np.random.default_rng(12)
    events = [("alive", [1] * n)]
    for g in range(60):
        m = int(rng.integers(1, 60))
        lines = []
        for q, k, v in zip(rng.integers(0, len(KINDS), m), rng.integers(0, 12, m), rng.integers(0, 900, m)):
            f = KINDS[q]
            lines.append(f % (k, v) if f.count(b"%d") == 2 else f % k if b"%d" in f else f)
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


def _replay(pkg, oracle, f, group, mode, sample, payloads, coalesce, rewrite=False):
    """The session through a core. rewrite: every batch is replaced by its thinned lines (the restatement's)."""
    core_mod = importlib.import_module("statsd-router_amd.core")
    core = core_mod.Core(f["n"], f["ds_hosts"], f["ds_data_ports"], f["ping_prefix"], f["hostname"], f["data_port"],
                         max_batch_bytes=1 << 20, log_level=f["log_level"])
    if payloads:
        core.set_payloads(True)
    if coalesce:
        core.set_coalesce(True)
    if sample:
        core.set_sample(pkg.SampleConfig(LIMIT, TYPES, 0, 0))
    alive = [0] * f["n"]
    pend = []
    hits = np.zeros((E.STEPS, 2), np.uint64)
    batches = [0]
    texts = []

    def flush_batch():
        if not pend:
            return
        framed = pkg.frame_datagrams(pend)
        if rewrite:
            if framed:
                recs, hashes, cnt = oracle.route(framed, f["n"], alive)
                res = E.apply(framed, recs[:cnt], hashes[:cnt], f["n"], LIMIT, TYPES, 0, batches[0])
                hits[:] += res.hits
                texts.append(res.text)
                framed = b"".join(E.lines_of(framed, res.text, res.out))
            {"copy": core.route, "async": core.submit, "slots": core.route}[mode](framed)
        elif mode == "slots":
            core.submit_slots(pend)
        else:
            sizes = [len(pkg.frame_datagrams([d])) for d in pend]
            ends = [int(x) for x, k in zip(np.cumsum(sizes), sizes) if k]   # empty datagrams have no entry
            {"copy": core.route, "async": core.submit}[mode](framed, ends)
        batches[0] += 1
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
    got_hits = core.sample_hits() if sample else None
    core.close()
    return core, final, got_hits, hits, texts


MODES = [(1, "copy"), (7, "async"), (1000, "async"), (7, "slots")]


@pytest.mark.parametrize("payloads,coalesce", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["lines", "payloads", "lines+coalesce", "payloads+coalesce"])
@pytest.mark.parametrize("group,mode", MODES)
def test_session(pkg, oracle, group, mode, payloads, coalesce):
    f = session()
    on, final_on, got_hits, _, _ = _replay(pkg, oracle, f, group, mode, True, payloads, coalesce)
    want, final_want, _, hits, texts = _replay(pkg, oracle, f, group, mode, False, payloads, coalesce, rewrite=True)
    off, _, _, _, _ = _replay(pkg, oracle, f, group, mode, False, payloads, coalesce)
    assert {k: v for k, v in on.packets.items() if v} == {k: v for k, v in want.packets.items() if v}
    assert final_on == final_want
    assert on.logs == off.logs                       # the WARN lines of the original batches, in their order
    assert got_hits.tolist() == hits.tolist()
    sent = b"".join(p for ps in on.packets.values() for p in ps)
    sent_off = b"".join(p for ps in off.packets.values() for p in ps)
    if group > 1:
        assert int(hits[1:, 0].sum()) > 300 and int(hits[1:, 1].sum()) > 20 and int(hits[0, 0]) > 100
        assert b"|ms|@0." in sent and b"|d|@0." in sent and b"|#env:p" in sent and len(sent) < len(sent_off)
        assert sum(x.count(b"\n") for x in texts) == int(hits[1:, 1].sum())
        if coalesce:
            assert b"core.req:" in sent and sent.count(b"core.plain.") < sent_off.count(b"core.plain.") + 1
    assert b"|@0.5\n" in sent and b"core.g." in sent and b"|@" not in sent_off.replace(b"|ms|@0.5\n", b"")


def test_switch_needs_an_idle_core_hits_reset_and_pings_are_exempt(pkg):
    core_mod = importlib.import_module("statsd-router_amd.core")
    with core_mod.Core(2, ["a", "b"], ["1", "2"], "p", "h", 9000, max_batch_bytes=1 << 16) as core:
        core.set_alive([1, 1])
        with pytest.raises(pkg.SrError) as ei:
            core.sample_hits()
        assert ei.value.errno == 22   # EINVAL: the switch was never on
        core.submit(b"k:1|ms\n" * 10)
        with pytest.raises(pkg.SrError) as ei:
            core.set_sample(pkg.SampleConfig(4))
        assert ei.value.errno == 16   # EBUSY: a batch is in flight
        core.drain()
        with pytest.raises(pkg.SrError) as ei:
            core.set_sample(pkg.SampleConfig(0))
        assert ei.value.errno == 22
        core.set_sample(pkg.SampleConfig(4))
        core.submit(b"k:5|ms\n" * 400 + b"j:1|ms\n" * 3 + b"c:1|c\n" * 50)
        core.ping()                    # drains; its own lines are never sampled and not counted
        got = core.sample_hits(reset=True)
        kept = sum(E.keep(E.name_hash(b"k"), 0, i, 6) for i in range(400))
        want = [[0, 0]] * E.STEPS
        want[0], want[6] = [3, 3], [400, kept]          # 400 <= 4 * 100: step 6; counters are not in the default types
        assert got.tolist() == want and 0 < kept < 20
        assert core.sample_hits().tolist() == [[0, 0]] * E.STEPS
        core.set_sample(None)
        core.route(b"k:5|ms\n" * 50)
        core.flush_timer()
        sent = b"".join(p for ps in core.packets.values() for p in ps)
        assert sent.count(b"k:5|ms\n") == 50 and sent.count(b"k:5|ms|@0.01\n") == kept and sent.count(b"j:1|ms\n") == 3
        assert sent.count(b"c:1|c\n") == 50
        assert any(l.startswith(b"p") for l in sent.split(b"\n"))   # the ping's lines went out
