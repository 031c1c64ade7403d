"""GPU: statsd-router-mi355x with SR_VALIDATE=<spec> end to end over loopback (the harness of
tests/test_gpu_router_e2e.py: the sink answers the downstreams' health checks and dumps every packet). With
SR_VALIDATE=drop the downstreams receive exactly the lines that the grammar keeps (tests/validate_expect.py), each
at its shard; the start-up INFO line repeats the spec; a bad spec ends the process with status 1 and one ERROR;
and with a ping interval of one second the per-ping line reports what was dropped, reason by reason."""
from __future__ import annotations

import os
import socket
import subprocess
import time
from collections import Counter

import numpy as np
import pytest

import validate_expect as E
from router_proc import OURS, Router, config_text, free_ports
from test_gpu_router_e2e import PREFIX as PING_PREFIX, SINK

pytestmark = pytest.mark.gpu

N_DS = 3
KINDS = [b"e2e.req.%d:%d|c", b"e2e.req.%d:%d|c", b"e2e.lat.%d:%d|ms|@0.5", b"e2e.g.%d:-%d|g|#env:p", b"e2e.bad.%d:x%d|c",
         b"e2e.q.%d:%d|q", b"e2e.nt.%d:%d", b"e2e.tag.%d:%d|c|#"]


def traffic():
    rng = np.random.default_rng(4)
    dgrams = []
    for j in range(200):
        lines = [KINDS[q] % (k, v) for q, k, v in zip(rng.integers(0, len(KINDS), 16), rng.integers(0, 9, 16),
                                                      rng.integers(0, 400, 16))]
        dgrams.append(b"\n".join(lines) + b"\n")
    return dgrams


def start(tmp, spec, ping, sink_idle="3.0"):
    base = free_ports(4 + 2 * N_DS)
    data_port, ctl, sink_base = base, base + 1, base + 4
    ds = [(sink_base + 2 * i, sink_base + 2 * i + 1) for i in range(N_DS)]
    dump = os.path.join(tmp, "dump.bin")
    sink = subprocess.Popen([SINK, str(sink_base), str(N_DS), "60", sink_idle, dump], stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE)
    assert sink.stderr.readline().strip() == b"ready"
    r = Router(OURS, config_text(data_port, ctl, ds, log_level=1, threads=1, flush=0.1, health=0.1, ping=ping,
                                 prefix=PING_PREFIX), tmp, env={"SR_VALIDATE": spec})
    return r, sink, data_port, dump


def test_the_downstreams_receive_exactly_the_kept_lines(tmp_path, oracle):
    dgrams = traffic()
    r, sink, data_port, dump = start(str(tmp_path), "drop", 1000.0)
    try:
        for i in range(N_DS):
            assert r.wait_for(lambda lv, m, i=i: m == b"ds_health_read_cb downstream %d is up" % i, 20), r.raw[-20:]
        time.sleep(0.3)   # the data thread has seen the alive bits
        s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        for d in dgrams:
            s.sendto(d, ("127.0.0.1", data_port))
            time.sleep(0.0005)
        s.close()
        sink.communicate(timeout=90)
    finally:
        r.stop()
        if sink.poll() is None:
            sink.kill()
    assert ("INFO", b"main: validate: drop") in r.lines
    assert [m for lv, m in r.lines if lv == "ERROR"] == []
    got = {i: Counter() for i in range(N_DS)}
    blob = open(dump, "rb").read()
    i = 0
    while i < len(blob):
        d, l = int.from_bytes(blob[i:i + 2], "little"), int.from_bytes(blob[i + 2:i + 4], "little")
        pkt = blob[i + 4:i + 4 + l]
        i += 4 + l
        for line in pkt.split(b"\n")[:-1]:
            if not line.startswith(PING_PREFIX.encode()):
                got[d][line + b"\n"] += 1
    want = {i: Counter() for i in range(N_DS)}
    sent = [l + b"\n" for d in dgrams for l in d.split(b"\n")[:-1]]
    dropped = 0
    for line in sent:
        if E.judge(line) == E.OK:
            want[oracle.find_downstream(oracle.hash_line(line), N_DS)][line] += 1
        else:
            dropped += 1
    assert got == want and dropped > 1000


@pytest.mark.parametrize("spec", ["dorp", "ok", "value,"])
def test_a_bad_spec_ends_the_process_with_status_1(tmp_path, spec):
    base = free_ports(4)
    cfg = config_text(base, base + 1, [(base + 2, base + 3)], log_level=1, threads=1)
    r = Router(OURS, cfg, str(tmp_path), env={"SR_VALIDATE": spec, "SR_REQUIRE_GPU": "0"})
    assert r.wait_exit(20) == 1
    errors = [m for lv, m in r.lines if lv == "ERROR"]
    assert len(errors) == 1 and b"SR_VALIDATE " + spec.encode() in errors[0]


def test_the_per_ping_line(tmp_path):
    """A ping interval of one second: after a datagram with 45 bad lines a ping logs what was dropped and the
    non-zero reasons in index order; the ping's own lines are not among them."""
    r, sink, data_port, _ = start(str(tmp_path), "value,type", 1.0, sink_idle="30.0")
    try:
        for i in range(N_DS):
            assert r.wait_for(lambda lv, m, i=i: m == b"ds_health_read_cb downstream %d is up" % i, 20), r.raw[-20:]
        assert ("INFO", b"main: validate: value,type") in r.lines
        time.sleep(0.3)
        s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        s.sendto(b"e2e.a:x|c\n" * 30 + b"e2e.b:1|q\n" * 10 + b"e2e.c:1|c|#\n" * 5 + b"e2e.req:1|c\n", ("127.0.0.1", data_port))
        s.close()
        want = b"validate: dropped lines=40 bytes=%d ok=1 type=10 value=30 tags=5" % (30 * 10 + 10 * 10)
        assert r.wait_for(lambda lv, m: lv == "INFO" and m == want, 8), [m for lv, m in r.lines if b"validate" in m]
    finally:
        r.stop()
        sink.kill()
