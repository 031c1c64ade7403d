"""GPU: statsd-router-mi355x with SR_NAME_RULES=<path> end to end over loopback (the harness of
tests/test_gpu_router_e2e.py: the sink answers the downstreams' health checks and dumps every packet). The
downstreams receive exactly the lines that the rule file keeps (tests/rules_expect.py), each at its shard; the
start-up INFO line names the rule count and the default; a bad file ends the process with a non-zero status and an
ERROR that names the offending line; and with a ping interval of one second the per-ping line reports what was
dropped."""
from __future__ import annotations

import os
import socket
import subprocess
import time
from collections import Counter

import numpy as np
import pytest

import rules_expect as E
from rules_expect import DROP, EXACT, KEEP, PREFIX
from router_proc import OURS, Router, config_text, free_ports
from test_gpu_router_e2e import PREFIX as PING_PREFIX, SINK

pytestmark = pytest.mark.gpu

N_DS = 3
FILE = b"# muted\ndrop e2e.debug.*\nkeep e2e.debug.keep.*\ndrop e2e.hot\n"
RULES = [(b"e2e.debug.", PREFIX, DROP), (b"e2e.debug.keep.", PREFIX, KEEP), (b"e2e.hot", EXACT, DROP)]


def traffic():
    rng = np.random.default_rng(4)
    dgrams = []
    for j in range(200):
        lines = []
        for u, k, v in zip(rng.random(16), rng.integers(0, 9, 16), rng.integers(0, 400, 16)):
            if u < 0.3:
                lines.append(b"e2e.hot:1|c")
            elif u < 0.5:
                lines.append(b"e2e.debug.t%d:%d|c" % (k, v))
            elif u < 0.6:
                lines.append(b"e2e.debug.keep.t%d:%d|c" % (k, v))
            elif u < 0.9:
                lines.append(b"e2e.req.%d:%d|c" % (k, v))
            else:
                lines.append(b"e2e.hot.%d:%d|ms" % (k, v))
        dgrams.append(b"\n".join(lines) + b"\n")
    return dgrams


def start(tmp, rules_text, ping, sink_idle="3.0"):
    base = free_ports(4 + 2 * N_DS)
    data_port, ctl, sink_base = base, base + 1, base + 4
    ds = [(sink_base + 2 * i, sink_base + 2 * i + 1) for i in range(N_DS)]
    dump = os.path.join(tmp, "dump.bin")
    path = os.path.join(tmp, "rules.txt")
    with open(path, "wb") as f:
        f.write(rules_text)
    sink = subprocess.Popen([SINK, str(sink_base), str(N_DS), "60", sink_idle, dump], stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE)
    assert sink.stderr.readline().strip() == b"ready"
    r = Router(OURS, config_text(data_port, ctl, ds, log_level=1, threads=1, flush=0.1, health=0.1, ping=ping,
                                 prefix=PING_PREFIX), tmp, env={"SR_NAME_RULES": path})
    return r, sink, data_port, dump


def test_the_downstreams_receive_exactly_the_kept_lines(tmp_path, oracle):
    dgrams = traffic()
    r, sink, data_port, dump = start(str(tmp_path), FILE, 1000.0)
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
    assert ("INFO", b"main: name_rules: 3 rules, default keep") in r.lines
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
        if [a for _, _, a in RULES + [(b"", 0, KEEP)]][E.match(RULES, line)] == KEEP:
            want[oracle.find_downstream(oracle.hash_line(line), N_DS)][line] += 1
        else:
            dropped += 1
    assert got == want and dropped > 1000


def test_a_bad_file_ends_the_process_and_names_the_line(tmp_path):
    base = free_ports(4)
    cfg = config_text(base, base + 1, [(base + 2, base + 3)], log_level=1, threads=1)
    bad = tmp_path / "bad.txt"
    bad.write_bytes(b"drop a.*\n# fine\nmute b\n")
    r = Router(OURS, cfg, str(tmp_path), env={"SR_NAME_RULES": str(bad), "SR_REQUIRE_GPU": "0"})
    assert r.wait_exit(20) != 0
    errors = [m for lv, m in r.lines if lv == "ERROR"]
    assert len(errors) == 1 and b"line 3" in errors[0] and str(bad).encode() in errors[0]
    r = Router(OURS, cfg, str(tmp_path), env={"SR_NAME_RULES": str(tmp_path / "missing.txt"), "SR_REQUIRE_GPU": "0"})
    assert r.wait_exit(20) != 0
    errors = [m for lv, m in r.lines if lv == "ERROR"]
    assert len(errors) == 1 and b"missing.txt" in errors[0]


def test_the_per_ping_line(tmp_path):
    """A ping interval of one second: after a datagram with 40 muted lines a ping logs what was dropped and the
    rules with the most hits."""
    r, sink, data_port, _ = start(str(tmp_path), FILE, 1.0, sink_idle="30.0")
    try:
        for i in range(N_DS):
            assert r.wait_for(lambda lv, m, i=i: m == b"ds_health_read_cb downstream %d is up" % i, 20), r.raw[-20:]
        time.sleep(0.3)
        s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        s.sendto(b"e2e.hot:1|c\n" * 30 + b"e2e.debug.x:1|c\n" * 10 + b"e2e.debug.keep.y:1|c\n" * 5 + b"e2e.req:1|c\n", ("127.0.0.1", data_port))
        s.close()
        want = b"name_rules: dropped lines=40 bytes=%d top: drop e2e.hot=30 drop e2e.debug.*=10 keep e2e.debug.keep.*=5" % (30 * 12 + 10 * 16)
        assert r.wait_for(lambda lv, m: lv == "INFO" and m == want, 8), [m for lv, m in r.lines if b"name_rules" in m]
    finally:
        r.stop()
        sink.kill()
