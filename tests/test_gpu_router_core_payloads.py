"""GPU: the router data thread with sr_core_set_payloads(1) replays the reference's scripted sessions
(tests/golden/router_*.json) exactly as without it (tests/test_gpu_router_core.py): every packet, log
line, pending buffer and counter, while every flushed packet reaches the emit callback as at most two
pieces, the bytes pending before the batch and one run of the device's arena."""
from __future__ import annotations

import importlib

import pytest

from conftest import load_router_fixture, router_fixtures

pytestmark = pytest.mark.gpu


def _framed_ends(pkg, dgrams):
    """The batch's framed bytes and each framed datagram's end offset (empty datagrams have none)."""
    ends, pos = [], 0
    for d in dgrams:
        k = len(pkg.frame_datagrams([d]))
        if k:
            pos += k
            ends.append(pos)
    return pkg.frame_datagrams(dgrams), ends


def _replay(pkg, f, group: int, mode: str):
    """tests/test_gpu_router_core.py's replay loop with the payload switch set."""
    core_mod = importlib.import_module("statsd-router_amd.core")
    core = core_mod.Core(f["n"], f["ds_hosts"], f["ds_data_ports"], f["ping_prefix"], f["hostname"], f["data_port"],
                         max_batch_bytes=1 << 20, log_level=f["log_level"])
    core.set_payloads(True)
    pend = []

    def flush_batch():
        if pend:
            framed, ends = _framed_ends(pkg, pend)
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
        elif e[0] == "flush":
            core.flush_timer()
        elif e[0] == "ping":
            core.ping()
    flush_batch()
    core.drain()
    final = {s: core.state(s) for s in range(f["n"])}
    core.close()
    return core, final


@pytest.mark.parametrize("group,mode", [(1, "copy"), (7, "copy"), (1000, "copy"), (1, "async"), (7, "async"),
                                        (1000, "async")])
@pytest.mark.parametrize("name", router_fixtures())
def test_core_replays_reference_session_from_the_arena(pkg, name, group, mode):
    f = load_router_fixture(name)
    core, final = _replay(pkg, f, group, mode)
    assert core.logs == f["logs"]
    assert {k: v for k, v in core.packets.items() if v} == f["packets"]
    assert final == f["final"]
    # the arena, not the line list: no packet came as more than the carried bytes and one run
    assert len(core.emit_iovecs) == sum(len(v) for v in core.packets.values())
    assert max(core.emit_iovecs, default=0) <= 2


def test_sessions_hold_packets_of_many_lines():
    """The two-piece bound above says something: the sessions flush packets of more than two lines."""
    most = max(p.count(b"\n") for name in router_fixtures() for v in load_router_fixture(name)["packets"].values()
               for p in v)
    assert most > 2


def test_set_payloads_needs_an_idle_core(pkg):
    core_mod = importlib.import_module("statsd-router_amd.core")
    with core_mod.Core(2, ["a", "b"], ["1", "2"], "p", "h", 9000, max_batch_bytes=1 << 16) as core:
        core.set_alive([1, 1])
        core.submit(b"k:1|c\n" * 10)
        with pytest.raises(pkg.SrError) as ei:
            core.set_payloads(True)
        assert ei.value.errno == 16   # EBUSY: a batch is in flight
        core.drain()
        core.set_payloads(True)
        core.submit(b"k:1|c\n" * 400)
        core.drain()
        core.set_payloads(False)
        core.flush_timer()
        assert b"".join(p for v in core.packets.values() for p in v).count(b"k:1|c\n") == 410
