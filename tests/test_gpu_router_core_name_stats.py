"""GPU: the router data thread with sr_core_set_name_stats replays the reference's scripted sessions
(tests/golden/router_*.json) exactly as without it: every packet, log line, pending buffer and counter; and the
snapshot it returns is the restatement's (tests/stats_expect.py) over the session's data lines, batch by batch,
through sr_core_route, sr_core_submit and sr_core_submit_slots. Ping lines are not counted."""
from __future__ import annotations

import importlib

import numpy as np
import pytest

import stats_expect as E
from conftest import load_router_fixture, router_fixtures

pytestmark = pytest.mark.gpu

CFG = dict(hll_p=6, cms_rows=3, cms_width=512, hot_slots=64, hot_div=50, hot_min_lines=2)


def _replay(pkg, oracle, f, group: int, mode: str, stats: bool):
    core_mod = importlib.import_module("statsd-router_amd.core")
    core = core_mod.Core(f["n"], f["ds_hosts"], f["ds_data_ports"], f["ping_prefix"], f["hostname"], f["data_port"],
                         max_batch_bytes=1 << 20, log_level=f["log_level"])
    if stats:
        core.set_name_stats(True, **CFG)
    want = E.Stats(f["n"], CFG)
    alive = [0] * f["n"]   # a core starts with every downstream dead
    pend = []

    def flush_batch():
        if not pend:
            return
        framed = pkg.frame_datagrams(pend)
        if mode == "slots":
            core.submit_slots(pend)
        else:
            sizes = [len(pkg.frame_datagrams([d])) for d in pend]
            ends = [int(x) for x, k in zip(np.cumsum(sizes), sizes) if k]   # empty datagrams have no entry
            {"copy": core.route, "async": core.submit}[mode](framed, ends)
        if framed:
            recs, hashes, cnt = oracle.route(framed, f["n"], alive)
            want.update([(framed, recs[:cnt], hashes[:cnt])])
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
    snaps = None
    if stats:
        first = core.name_stats(reset=True)
        snaps = (first, core.name_stats())
    core.close()
    return core, final, snaps, want.read()


@pytest.mark.parametrize("group,mode", [(1, "copy"), (7, "copy"), (1000, "async"), (7, "async"), (1, "slots"),
                                        (7, "slots"), (200, "slots")])
@pytest.mark.parametrize("name", router_fixtures())
def test_core_session_with_name_stats(pkg, oracle, name, group, mode):
    f = load_router_fixture(name)
    core, final, (snap, after), want = _replay(pkg, oracle, f, group, mode, True)
    # outputs unchanged: the fixture is what the switch-off replay gives (tests/test_gpu_router_core.py)
    assert core.logs == f["logs"]
    assert {k: v for k, v in core.packets.items() if v} == f["packets"]
    assert final == f["final"]
    assert E.same(snap, want) == [], E.same(snap, want)
    lines = sum(pkg.frame_datagrams([e[1]]).count(b"\n") for e in f["events"] if e[0] == "dgram")
    assert int(snap.lines.sum()) + int(snap.ignored) == lines and snap.ignored == 0
    # read with reset, then a second read: zeros
    assert int(after.lines.sum()) == 0 and after.n_hot == 0 and not after.cells.any() and not after.regs.any()
    assert not after.shard_lines.any() and after.hot_overflow == 0


def test_sessions_have_hot_names(pkg, oracle):
    """The comparison above says something: some session lists hot names, and valid lines are counted."""
    hot = valid = 0
    for name in router_fixtures():
        _, _, (snap, _), want = _replay(pkg, oracle, load_router_fixture(name), 7, "copy", True)
        hot += snap.n_hot
        valid += int(snap.lines[0])
    assert hot > 0 and valid > 0


def test_switch_needs_an_idle_core_and_can_be_turned_off(pkg):
    core_mod = importlib.import_module("statsd-router_amd.core")
    with core_mod.Core(2, ["a", "b"], ["1", "2"], "p", "h", 9000, max_batch_bytes=1 << 16) as core:
        with pytest.raises(pkg.SrError) as ei:
            core.name_stats()
        assert ei.value.errno == 22   # EINVAL: never switched on
        core.set_alive([1, 1])
        core.submit(b"k:1|c\n" * 10)
        with pytest.raises(pkg.SrError) as ei:
            core.set_name_stats(True)
        assert ei.value.errno == 16   # EBUSY: a batch is in flight
        core.drain()
        core.set_name_stats(True, **CFG)
        core.submit(b"k:1|c\n" * 400)
        core.ping()                    # drains; its own lines are not counted
        assert int(core.name_stats().lines[0]) == 400
        core.set_name_stats(False)
        core.submit(b"k:1|c\n" * 50)
        snap = core.name_stats()
        assert int(snap.lines[0]) == 400 and [bytes(e["name"][:1]) for e in snap.hot] == [b"k"]
