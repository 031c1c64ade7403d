"""GPU: statsd-router-mi355x with SR_COALESCE=1 end to end over loopback (the harness of
tests/test_gpu_router_e2e.py: the sink answers the downstreams' health checks and dumps every packet).

Exact case: one datagram is always one batch, so 50 lines of one counter in one datagram reach their downstream as
one line with the sum, and the datagram's other lines unchanged. Conservation case: many datagrams; which lines
meet in a batch depends on how recvmmsg groups them, so only what every grouping conserves is checked: the sum per
name at each downstream, and the multiset of the lines that are no plain counters."""
from __future__ import annotations

import os
import socket
import subprocess
import time
from collections import Counter

import numpy as np
import pytest

import coalesce_expect as E
from router_proc import OURS, Router, config_text, free_ports
from test_gpu_router_e2e import PREFIX, SINK

pytestmark = pytest.mark.gpu

N_DS = 3


def run_router(datagrams, tmp, env):
    base = free_ports(4 + 2 * N_DS)
    data_port, ctl, sink_base = base, base + 1, base + 4
    ds = [(sink_base + 2 * i, sink_base + 2 * i + 1) for i in range(N_DS)]
    dump = os.path.join(tmp, "dump.bin")
    sink = subprocess.Popen([SINK, str(sink_base), str(N_DS), "60", "3.0", dump], stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE)
    assert sink.stderr.readline().strip() == b"ready"
    r = Router(OURS, config_text(data_port, ctl, ds, log_level=1, threads=1, flush=0.1, health=0.1, ping=1000.0,
                                 prefix=PREFIX), tmp, env=env)
    try:
        for i in range(N_DS):
            assert r.wait_for(lambda lv, m, i=i: m == b"ds_health_read_cb downstream %d is up" % i, 20), r.raw[-20:]
        time.sleep(0.3)   # the data thread has seen the alive bits
        s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        for d in datagrams:
            s.sendto(d, ("127.0.0.1", data_port))
            time.sleep(0.0005)
        s.close()
        sink.communicate(timeout=90)
    finally:
        r.stop()
        if sink.poll() is None:
            sink.kill()
    got = {i: [] for i in range(N_DS)}
    with open(dump, "rb") as f:
        blob = f.read()
    i = 0
    while i < len(blob):
        d, l = int.from_bytes(blob[i:i + 2], "little"), int.from_bytes(blob[i + 2:i + 4], "little")
        pkt = blob[i + 4:i + 4 + l]
        i += 4 + l
        assert len(pkt) <= 1450 and pkt.endswith(b"\n")
        got[d] += [line + b"\n" for line in pkt.split(b"\n")[:-1] if not line.startswith(PREFIX.encode())]
    errors = [m for lv, m in r.lines if lv == "ERROR"]
    return got, errors


def shard_of(oracle, line):
    return oracle.find_downstream(oracle.hash_line(line), N_DS)


def test_one_datagram_is_one_batch(tmp_path, oracle):
    others = [b"e2e.other.a:7|c", b"e2e.timer:12|ms", b"e2e.other.b:3|c|@0.5", b"e2e.gauge:1.5|g"]
    lines = [b"e2e.hot:1|c"] * 25 + others[:2] + [b"e2e.hot:1|c"] * 25 + others[2:]
    got, errors = run_router([b"\n".join(lines) + b"\n"], str(tmp_path), {"SR_COALESCE": "1"})
    assert errors == []
    want = {i: Counter() for i in range(N_DS)}
    for line in [b"e2e.hot:50|c"] + others:
        want[shard_of(oracle, line + b"\n")][line + b"\n"] += 1
    assert {k: Counter(v) for k, v in got.items()} == want   # e2e.hot:50|c once, every other line unchanged


def test_many_datagrams_conserve_sums_and_other_lines(tmp_path, oracle):
    rng = np.random.default_rng(4)
    dgrams = []
    for j in range(300):
        lines = []
        for u, k, v in zip(rng.random(16), rng.integers(0, 9, 16), rng.integers(-20, 400, 16)):
            if u < 0.55:
                lines.append(b"e2e.hot:1|c")
            elif u < 0.8:
                lines.append(b"e2e.req.%d:%d|c" % (k, v))
            elif u < 0.92:
                lines.append(b"e2e.lat.%d:%d|ms" % (k, abs(v)))
            else:
                lines.append(b"e2e.req.%d:%d|c|@0.1" % (k, abs(v)))
        dgrams.append(b"\n".join(lines) + b"\n")
    got, errors = run_router(dgrams, str(tmp_path), {"SR_COALESCE": "1"})
    assert errors == []
    sent = [(shard_of(oracle, l + b"\n"), l + b"\n") for d in dgrams for l in d.split(b"\n")[:-1]]
    want_sums, want_rest = E.ledger(sent)
    got_sums, got_rest = E.ledger((k, l) for k, ls in got.items() for l in ls)
    assert got_sums == want_sums
    assert Counter(got_rest) == Counter(want_rest)
    n_in = sum(1 for _, l in sent if E.parse(l) is not None)
    n_out = sum(1 for ls in got.values() for l in ls if l.count(b"|c\n") and b"@" not in l)
    assert n_out < n_in // 2     # it did coalesce: a datagram alone holds each of its names once at most
