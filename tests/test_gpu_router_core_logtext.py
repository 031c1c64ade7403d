"""GPU: the router core with its batches' log text written on the device (sr_core_set_device_log) replays
the scripted sessions the compiled reference ran (tests/golden/router_*.json): logs, packets and final state
are the fixture's, with 1, 7 and 1000 datagrams a batch, synchronous, double-buffered and from slots, with and
without datagram ends; at log_level 0 also against the oracle's restatement of the reference data thread for
the sessions recorded at WARN; with an arena so small that every batch falls back to the host formatter; and
in block mode, where a batch's text arrives in one call between the host's own messages."""
from __future__ import annotations

import importlib

import pytest

from conftest import load_router_fixture, router_fixtures

pytestmark = pytest.mark.gpu

ARENA_SLOTS = 200
PFX = (b"2026-01-01 00:00:00 12345 TRACE ", b"2026-01-01 00:00:00 12345 WARN ")


def _framed_ends(pkg, dgrams):
    ends, pos = [], 0
    for d in dgrams:
        k = len(pkg.frame_datagrams([d]))
        if k:
            pos += k
            ends.append(pos)
    return pkg.frame_datagrams(dgrams), ends


def _replay(pkg, f, events, group, mode, *, level=None, with_ends=True, text_cap=0, prefixes=None, device_log=True):
    core_mod = importlib.import_module("statsd-router_amd.core")
    core = core_mod.Core(f["n"], f["ds_hosts"], f["ds_data_ports"], f["ping_prefix"], f["hostname"], f["data_port"],
                         max_batch_bytes=ARENA_SLOTS * 4096, log_level=f["log_level"] if level is None else level)
    if device_log:
        core.set_device_log(True, text_cap, prefixes)
    pend = []
    if mode == "slots":
        group = min(group, ARENA_SLOTS)

    def flush_batch():
        if pend:
            if mode == "slots":
                core.submit_slots(pend)
            else:
                framed, ends = _framed_ends(pkg, pend)
                {"copy": core.route, "async": core.submit}[mode](framed, ends if with_ends else None)
            pend.clear()

    for e in events:
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
    core.stats = core.device_log_stats()   # (batches logged from the device's text, batches the host formatted)
    core.close()
    return core, final


def _data_messages(logs):
    return sum(m.startswith((b"udp_read_cb:", b"process_data_line:")) for _, m in logs)


def _oracle_run(f, events, level):
    import sr_router_oracle as RO

    t = RO.DataThread(f["n"], f["ds_hosts"], f["ds_data_ports"], f["ping_prefix"], f["hostname"], f["data_port"],
                      log_level=level)
    return t.run(events)


@pytest.mark.parametrize("mode", ["copy", "async", "slots"])
@pytest.mark.parametrize("group", [1, 7, 1000])
@pytest.mark.parametrize("name", router_fixtures())
def test_core_replays_reference_session_with_device_log(pkg, name, group, mode):
    f = load_router_fixture(name)
    core, final = _replay(pkg, f, f["events"], group, mode)
    assert core.logs == f["logs"]
    assert {k: v for k, v in core.packets.items() if v} == f["packets"]
    assert final == f["final"]
    assert core.stats[0] > 0 and core.stats[1] == 0   # every batch's messages came from the device's text


@pytest.mark.parametrize("mode", ["copy", "async"])
@pytest.mark.parametrize("group", [1, 7, 1000])
def test_trace_core_without_datagram_ends(pkg, group, mode):
    name = [n for n in router_fixtures() if load_router_fixture(n)["log_level"] == 0][0]
    f = load_router_fixture(name)
    core, final = _replay(pkg, f, f["events"], group, mode, with_ends=False)
    assert core.logs == [(lv, m) for lv, m in f["logs"] if not m.startswith(b"udp_read_cb: got packet ")]
    assert {k: v for k, v in core.packets.items() if v} == f["packets"]
    assert final == f["final"]


@pytest.mark.parametrize("mode", ["copy", "async", "slots"])
@pytest.mark.parametrize("name", router_fixtures())
def test_sessions_at_trace_against_the_oracle(pkg, name, mode):
    """Every session at log_level 0, also those recorded at WARN: the oracle's restatement of the reference
    data thread (pinned to the golden files by tests/test_oracle_router.py) says what a TRACE router logs."""
    f = load_router_fixture(name)
    t = _oracle_run(f, f["events"], 0)
    core, final = _replay(pkg, f, f["events"], 7, mode, level=0)
    assert core.logs == t.logs
    assert core.stats[0] > 0 and core.stats[1] == 0
    assert {k: v for k, v in core.packets.items() if v} == {k: v for k, v in t.packets.items() if v}
    assert final == t.final()


@pytest.mark.parametrize("mode", ["copy", "async", "slots"])
@pytest.mark.parametrize("group", [1, 7, 1000])
@pytest.mark.parametrize("name", router_fixtures())
def test_every_batch_falls_back_when_the_arena_is_tiny(pkg, name, group, mode):
    f = load_router_fixture(name)
    core, final = _replay(pkg, f, f["events"], group, mode, text_cap=16)
    assert core.logs == f["logs"]
    # a 16-byte arena holds no message: only batches without one are served by the device
    assert core.stats[1] > 0 or _data_messages(f["logs"]) == 0
    assert {k: v for k, v in core.packets.items() if v} == f["packets"]
    assert final == f["final"]


def _render(logs, prefixes, max_msg=2047):
    """Host messages as the executable writes them; block entries are on the wire already."""
    out = []
    for lv, text in logs:
        out.append(text if lv < 0 else (prefixes[1 if lv >= 3 else 0] + text)[:max_msg] + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("mode", ["copy", "async", "slots"])
@pytest.mark.parametrize("name", router_fixtures())
def test_block_mode(pkg, name, mode):
    f = load_router_fixture(name)
    core, final = _replay(pkg, f, f["events"], 7, mode, prefixes=PFX)
    assert _render(core.logs, PFX) == _render(f["logs"], PFX)
    host = [m for m in core.logs if m[0] >= 0]
    assert core.stats[1] == 0 and (core.blocks or _data_messages(f["logs"]) == 0)
    assert sum(n for _, n in core.blocks) + len(host) == len(f["logs"])
    assert all(n > 0 and text.endswith(b"\n") for text, n in core.blocks)
    assert {k: v for k, v in core.packets.items() if v} == f["packets"]
    assert final == f["final"]


def test_block_mode_cuts_long_messages_and_keeps_host_messages_in_place(pkg):
    """A 4095-byte datagram that is one invalid line, a valid line of 1449 bytes and NULs, at log_level 0 with
    every downstream of the last batch dead; pings between the batches. Messages over 2047 bytes are cut."""
    f = load_router_fixture([n for n in router_fixtures() if load_router_fixture(n)["log_level"] == 0][0])
    n = f["n"]
    events = [("alive", [1] * n), ("dgram", b"J" * 4095), ("dgram", b"v" * 1443 + b":1|c\n" + b"cut\0here:1|c\nnocolon\0x\n"),
              ("ping",), ("dgram", b"a:1|c\n" * 100), ("dgram", b""), ("dgram", b"\n" * 40), ("flush",),
              ("alive", [0] * n), ("dgram", b"dead.now:1|c\nb:2|c"), ("ping",)]
    t = _oracle_run(f, events, 0)
    assert max(len(m) for _, m in t.logs) > 4000
    for mode in ("copy", "async", "slots"):
        core, final = _replay(pkg, f, events, 3, mode, level=0, prefixes=PFX)
        assert _render(core.logs, PFX) == _render(t.logs, PFX), mode
        kinds = [lv < 0 for lv, _ in core.logs]
        assert True in kinds and False in kinds and kinds.index(False) > kinds.index(True)   # pings after a block
        assert {k: v for k, v in core.packets.items() if v} == {k: v for k, v in t.packets.items() if v}
        assert final == t.final()


@pytest.mark.parametrize("mode", ["copy", "async"])
@pytest.mark.parametrize("prefixes", [None, PFX], ids=["message", "block"])
def test_more_datagrams_than_the_staging_holds_are_still_routed(pkg, mode, prefixes):
    """A host-framed batch of more than SR_MAX_SLOTS datagrams at log_level 0: its ends cannot be staged, so
    the host formats that batch; it is routed like any other, and the batches around it come from the device."""
    f = load_router_fixture([n for n in router_fixtures() if load_router_fixture(n)["log_level"] == 0][0])
    n = f["n"]
    many = pkg.SR_MAX_SLOTS + 3
    events = [("alive", [1] * n), ("dgram", b"before:1|c\nnocolon\n"), ("flush",)]
    events += [("dgram", b"a:%d|c" % (i % 10)) for i in range(many)]
    events += [("flush",), ("dgram", b"after:1|c"), ("flush",)]
    t = _oracle_run(f, events, 0)
    assert len(t.logs) == 3 * many + 7
    core, final = _replay(pkg, f, events, 100000, mode, level=0, prefixes=prefixes)
    if prefixes is None:
        assert core.logs == t.logs
    else:
        assert _render(core.logs, PFX) == _render(t.logs, PFX)
        assert len(core.blocks) == 2
    assert core.stats == (2, 1)
    assert {k: v for k, v in core.packets.items() if v} == {k: v for k, v in t.packets.items() if v}
    assert final == t.final()


def test_switch_rules(pkg):
    core_mod = importlib.import_module("statsd-router_amd.core")
    f = load_router_fixture(router_fixtures()[0])
    core = core_mod.Core(f["n"], f["ds_hosts"], f["ds_data_ports"], f["ping_prefix"], f["hostname"], f["data_port"],
                         max_batch_bytes=1 << 16)
    core.set_alive([1] * f["n"])
    core.submit(b"a:1|c\n")
    with pytest.raises(pkg.SrError) as e:
        core.set_device_log(True)
    assert e.value.errno == 16   # EBUSY: a batch is in flight
    core.drain()
    core.set_device_log(True)
    core.route(b"nocolon\n")
    core.set_device_log(False)
    core.route(b"nocolon2\n")
    assert core.logs == [(3, b"process_data_line: invalid metric nocolon"), (3, b"process_data_line: invalid metric nocolon2")]
    core.close()
