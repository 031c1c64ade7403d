"""GPU: statsd-router-mi355x with SR_NAME_STATS=1 at log_level 2 end to end over loopback: after the ping tick
that follows a fixed set of datagrams the data thread logs exactly the lines the restatement's snapshot
(tests/stats_expect.py) prescribes; without the variable it logs no name_stats line. Same harness as
tests/test_gpu_router_e2e.py (the sink answers the downstreams' health checks).

The batches the data thread forms depend on when the datagrams arrive, so the input is made indifferent to them:
every datagram carries the same two heavy names, the threshold stays at hot_min_lines (1024) for the whole run,
and a name is hot under every batching iff its final estimate reaches it and it is in the last datagram; the
test checks on the restatement that no other name comes near.

Nothing here depends on the wall clock. A window between two ping ticks is opened by a tick's own report: the
test sends one probe line, waits for the report that counts it (the statistics start again there) and sends the
datagrams at once, which takes a fraction of the ping interval. Should a tick still fall among them (a loaded
machine), that window's report is not the expected one and the window is tried again, a few times."""
from __future__ import annotations

import math
import os
import socket
import subprocess
import time

import pytest

import stats_expect as E
from router_proc import OURS, Router, config_text, free_ports
from test_gpu_router_e2e import PREFIX, SINK

pytestmark = pytest.mark.gpu

N_DS = 3
PING = 1.0        # seconds between ping ticks
SINK_IDLE = 5.0


def _datagrams():
    out = []
    for j in range(200):
        lines = [b"api.requests.total:1|c"] * 10 + [b"db.query.time:%d|ms" % (j % 50)] * 6
        lines += [b"host%d.cpu.%d:%d|g" % (j, k, k) for k in range(4)] + [b"bad line %d" % j]
        out.append(b"\n".join(lines) + b"\n")
    return out


def _expected(oracle, pkg):
    dg = _datagrams()
    framed = pkg.frame_datagrams(dg)
    recs, hashes, cnt = oracle.route(framed, N_DS, [1] * N_DS)
    st = E.Stats(N_DS, None)
    st.update([(framed, recs[:cnt], hashes[:cnt])])
    snap = st.read()
    assert st.threshold() == 1024 and snap.total == 200 * 20 and int(snap.lines[2]) == 200
    # batching cannot matter: the hot names are in every datagram, nothing else is within reach of the threshold
    names = [bytes(e["name"][: e["name_len"]]) for e in snap.hot]
    assert names == [b"api.requests.total", b"db.query.time"] and not snap.hot_overflow
    last = set(l.split(b":")[0] for l in dg[-1].split(b"\n") if b":" in l)
    assert set(names) <= last
    colder = [E.estimate(snap, E.name_hash(b"host%d.cpu.%d" % (j, k))) for j in range(200) for k in range(4)]
    assert max(colder) < 512
    lines = [b"name_stats: lines=%d names~%d hot=%d" % (snap.total, math.floor(E.cardinality(snap) + 0.5), len(snap.hot))]
    lines += [b"name_stats: hot %s lines~%d" % (nm, int(e["lines"])) for nm, e in zip(names, snap.hot)]
    return lines


def _start(tmp, log_level, env):
    base = free_ports(4 + 2 * N_DS)
    data_port, ctl, sink_base = base, base + 1, base + 4
    ds = [(sink_base + 2 * i, sink_base + 2 * i + 1) for i in range(N_DS)]
    # the sink ends after SINK_IDLE seconds without data, and with it the downstreams' health: far above the
    # longest pause of a test (two ping intervals and a flush)
    sink = subprocess.Popen([SINK, str(sink_base), str(N_DS), "60", str(SINK_IDLE), os.path.join(tmp, "dump.bin")],
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert sink.stderr.readline().strip() == b"ready"
    r = Router(OURS, config_text(data_port, ctl, ds, log_level=log_level, threads=1, flush=0.1, health=0.1, ping=PING,
                                 prefix=PREFIX), tmp, env=env)
    return r, sink, data_port


def _stats_lines(r):
    with r._cv:
        return [m for lv, m in r.lines if m.startswith(b"name_stats:")]


def _headers(r):
    return sum(m.startswith(b"name_stats: lines=") for m in _stats_lines(r))


def _next_report(r, s, port, timeout, repeat=False):
    """Returns once a tick's report is logged that was not there before, i.e. right behind a tick, with the
    statistics started again. One probe line makes sure that the tick has something to report; repeat sends one
    every 50 ms, for the start, when lines do not count until the downstreams are up."""
    n0, end = _headers(r), time.monotonic() + timeout
    s.sendto(b"probe.line:1|c\n", ("127.0.0.1", port))
    while _headers(r) == n0:
        assert time.monotonic() < end and r.p.poll() is None, r.raw[-20:]
        with r._cv:
            r._cv.wait(0.05)
        if repeat and _headers(r) == n0:
            s.sendto(b"probe.line:1|c\n", ("127.0.0.1", port))


def _wait(r, done, seconds):
    end = time.monotonic() + seconds
    while not done() and time.monotonic() < end:
        with r._cv:
            r._cv.wait(0.02)
    return done()


def test_name_stats_lines_after_one_ping_tick(pkg, oracle, tmp_path):
    want = _expected(oracle, pkg)
    r, sink, port = _start(str(tmp_path), 2, {"SR_NAME_STATS": "1"})
    s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    tried = []
    try:
        _next_report(r, s, port, 30, repeat=True)    # the downstreams are up and the data thread routes
        for _ in range(5):
            # probes of the start that came behind their tick, or what a failed attempt left, belong to the window
            # now open: one more report takes them out of the way
            _next_report(r, s, port, 3 * PING)
            n0 = _headers(r)
            for d in _datagrams():
                s.sendto(d, ("127.0.0.1", port))
                time.sleep(0.0005)
            assert _wait(r, lambda: _headers(r) > n0, 3 * PING), _stats_lines(r)[-6:]   # the window's report
            lines = _stats_lines(r)
            at = [i for i, m in enumerate(lines) if m.startswith(b"name_stats: lines=")][n0]
            _wait(r, lambda: len(_stats_lines(r)) >= at + len(want), 0.5)   # its other lines follow at once
            got = _stats_lines(r)[at: at + len(want)]
            tried.append(got)
            if got == want:
                break
        with r._cv:
            levels = {lv for lv, m in r.lines if m.startswith(b"name_stats:")}
    finally:
        s.close()
        r.stop()
        sink.kill()
    assert tried[-1] == want, tried
    assert levels == {"INFO"}


def test_no_name_stats_line_without_the_variable(tmp_path, monkeypatch):
    monkeypatch.delenv("SR_NAME_STATS", raising=False)
    r, sink, port = _start(str(tmp_path), 1, None)   # log_level 1: the health checker says when the downstreams are up
    s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    try:
        for i in range(N_DS):
            assert r.wait_for(lambda lv, m, i=i: m == b"ds_health_read_cb downstream %d is up" % i, 20), r.raw[-20:]
        for d in _datagrams():
            s.sendto(d, ("127.0.0.1", port))
        last = b"process_data_line: invalid metric bad line 199"
        assert r.wait_for(lambda lv, m: m == last, 10), r.raw[-5:]    # every datagram is routed
        time.sleep(PING + 0.2)      # any interval of this length holds a ping tick: the one that would report them
        got = _stats_lines(r)
        with r._cv:
            routed = [m for lv, m in r.lines if m.startswith(b"process_data_line: invalid metric bad line")]
    finally:
        s.close()
        r.stop()
        sink.kill()
    assert got == [] and len(routed) == 200
