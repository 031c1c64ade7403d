"""GPU: statsd-router-mi355x with SR_SAMPLE=<spec> end to end over loopback (the harness of
tests/test_gpu_router_e2e.py: the sink answers the downstreams' health checks and dumps every packet). Datagrams sent
one at a time are batches of their own, thinned under the seeds 0, 1, 2 and so on: with SR_SAMPLE=4 the downstreams
receive exactly the lines that tests/sample_expect.py leaves of them, rewritten ones with their rate, each at its
shard; the start-up INFO line repeats the spec; a bad spec ends the process with status 1 and one ERROR; and with a
ping interval of one second the per-ping line reports what was seen and dropped, rate by rate."""
from __future__ import annotations

import os
import socket
import subprocess
import time
from collections import Counter

import numpy as np
import pytest

import sample_expect as E
from router_proc import OURS, Router, config_text, free_ports
from test_gpu_router_e2e import PREFIX as PING_PREFIX, SINK

pytestmark = pytest.mark.gpu

N_DS = 3
KINDS = [b"e2e.time:%d%d|ms", b"e2e.time:%d.%d|ms|#env:p", b"e2e.hist.%d:%d|h", b"e2e.req:%d%d|c", b"e2e.lat.%d:%d|ms|@0.5",
         b"e2e.g.%d:-%d|g", b"e2e.dist:%d%d|d", b"e2e.cold.%d:%d|ms"]


def traffic():
    rng = np.random.default_rng(4)
    dgrams = []
    for j in range(12):
        lines = [KINDS[q] % (k, v) for q, k, v in zip(rng.integers(0, len(KINDS), 150), rng.integers(0, 40, 150),
                                                      rng.integers(0, 400, 150))]
        dgrams.append(b"\n".join(lines) + b"\n")
        assert len(dgrams[-1]) < 4000
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
                                 prefix=PING_PREFIX), tmp, env={"SR_SAMPLE": spec})
    return r, sink, data_port, dump


def test_the_downstreams_receive_exactly_the_thinned_lines(tmp_path, oracle):
    dgrams = traffic()
    r, sink, data_port, dump = start(str(tmp_path), "4", 1000.0)
    try:
        for i in range(N_DS):
            assert r.wait_for(lambda lv, m, i=i: m == b"ds_health_read_cb downstream %d is up" % i, 20), r.raw[-20:]
        time.sleep(0.3)   # the data thread has seen the alive bits
        s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        for d in dgrams:
            s.sendto(d, ("127.0.0.1", data_port))
            time.sleep(0.05)   # each datagram is read, routed and thinned before the next arrives: a batch of its own
        s.close()
        sink.communicate(timeout=90)
    finally:
        r.stop()
        if sink.poll() is None:
            sink.kill()
    assert ("INFO", b"main: sample: 4") in r.lines
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
    dropped = rewritten = 0
    for seed, d in enumerate(dgrams):
        recs, hashes, cnt = oracle.route(np.frombuffer(d, np.uint8), N_DS, [1] * N_DS)
        res = E.apply(d, recs[:cnt], hashes[:cnt], N_DS, 4, E.TYPES_DEFAULT, 0, seed)
        for rec, line in zip(res.out, E.lines_of(d, res.text, res.out)):
            want[int(rec["route"])][line] += 1
        dropped += int(res.counts[1])
        rewritten += int(res.counts[2])
    assert got == want and dropped > 300 and rewritten > 50
    sent = b"".join(k for c in got.values() for k in c)
    assert b"|ms|@0." in sent and b"|d|@0." in sent and b"|c|@" not in sent   # counters are not in the default types


@pytest.mark.parametrize("spec", ["0", "four", "4:", "4:g", "4:ms,"])
def test_a_bad_spec_ends_the_process_with_status_1(tmp_path, spec):
    base = free_ports(4)
    cfg = config_text(base, base + 1, [(base + 2, base + 3)], log_level=1, threads=1)
    r = Router(OURS, cfg, str(tmp_path), env={"SR_SAMPLE": spec, "SR_REQUIRE_GPU": "0"})
    assert r.wait_exit(20) == 1
    errors = [m for lv, m in r.lines if lv == "ERROR"]
    assert len(errors) == 1 and b"SR_SAMPLE " + spec.encode() in errors[0]


def test_the_per_ping_line(tmp_path):
    """A ping interval of one second: after a datagram with 45 lines of one timer, 11 of one histogram, 3 of another
    and 20 counters under `4:ms,h` a ping logs what was seen and dropped and the steps that were taken in order; the
    ping's own lines are not among them."""
    r, sink, data_port, _ = start(str(tmp_path), "4:ms,h", 1.0, sink_idle="30.0")
    try:
        for i in range(N_DS):
            assert r.wait_for(lambda lv, m, i=i: m == b"ds_health_read_cb downstream %d is up" % i, 20), r.raw[-20:]
        assert ("INFO", b"main: sample: 4:ms,h") in r.lines
        time.sleep(0.3)
        lines = [b"e2e.a:%d|ms\n" % i for i in range(45)] + [b"e2e.b:1|h\n"] * 11 + [b"e2e.c:1|h\n"] * 3 + [b"e2e.d:1|c\n"] * 20
        s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        s.sendto(b"".join(lines), ("127.0.0.1", data_port))
        s.close()
        ka = sum(E.keep(E.name_hash(b"e2e.a"), 0, i, 4) for i in range(45))          # 45 <= 4 * 20: step 4
        kb = sum(E.keep(E.name_hash(b"e2e.b"), 0, i, 2) for i in range(45, 56))      # 11 <= 4 * 5: step 2
        want = b"sample: seen=59 dropped=%d 0.2=11/%d 0.05=45/%d" % (56 - ka - kb, kb, ka)
        assert r.wait_for(lambda lv, m: lv == "INFO" and m == want, 8), [m for lv, m in r.lines if b"sample" in m]
    finally:
        r.stop()
        sink.kill()
