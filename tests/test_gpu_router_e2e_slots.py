"""GPU: statsd-router-mi355x with SR_DEVICE_FRAMING=1 end to end over loopback: datagrams stay in their
recvmmsg slots and are framed on the GPU (sr_core_submit_slots). Same harness and checks as
tests/test_gpu_router_e2e.py: per downstream, the received data lines are what the reference's data thread
(oracle restatement) pushes there, and the WARN lines are the reference's texts, in order. The catalogue is
that test's, plus what framing is about: datagrams without a final '\\n', empty ones, and one longer than
recv()'s 4095 bytes."""
from __future__ import annotations

import os
import random
import socket
import subprocess
import time
from collections import Counter

import pytest

from router_proc import OURS, Router, config_text, free_ports
from test_gpu_router_e2e import PREFIX, SINK, catalogue, expected, valid_metric

pytestmark = pytest.mark.gpu


def framing_catalogue():
    r = random.Random(77)
    dg = catalogue(seed=21)[:300]
    extra = [valid_metric(r, n) for n in (20, 64, 1024)]                            # no final '\n'
    extra += [b"\n".join(valid_metric(r, 100) for _ in range(5)) for _ in range(20)]  # several lines, the last open
    extra += [b"", b"\n", b"", b"x"]
    extra += [b"\n".join(valid_metric(r, 200) for _ in range(30))]                  # 6029 bytes: cut at 4095
    for i, d in enumerate(extra):
        dg.insert(7 * i + 3, d)
    return dg


def run_router_framing(datagrams, n_ds, tmp):
    base = free_ports(4 + 2 * n_ds)
    data_port, ctl, sink_base = base, base + 1, base + 4
    ds = [(sink_base + 2 * i, sink_base + 2 * i + 1) for i in range(n_ds)]
    dump = os.path.join(tmp, "dump-framing.bin")
    sink = subprocess.Popen([SINK, str(sink_base), str(n_ds), "60", "3.0", dump], stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE)
    assert sink.stderr.readline().strip() == b"ready"
    r = Router(OURS, config_text(data_port, ctl, ds, log_level=1, threads=1, flush=0.1, health=0.1, ping=1000.0,
                                 prefix=PREFIX), tmp, env={"SR_DEVICE_FRAMING": "1"})
    try:
        for i in range(n_ds):
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
    got = {i: Counter() for i in range(n_ds)}
    with open(dump, "rb") as f:
        blob = f.read()
    i = 0
    while i < len(blob):
        d, l = int.from_bytes(blob[i:i + 2], "little"), int.from_bytes(blob[i + 2:i + 4], "little")
        pkt = blob[i + 4:i + 4 + l]
        i += 4 + l
        assert len(pkt) <= 1450 and pkt.endswith(b"\n")
        for line in pkt.split(b"\n")[:-1]:
            if not line.startswith(PREFIX.encode()):
                got[d][line + b"\n"] += 1
    data_path = (b"udp_read_cb:", b"process_data_line:", b"find_downstream:")
    return got, [m for lv, m in r.lines if lv == "WARN" and m.startswith(data_path)]


def test_router_end_to_end_with_device_framing(tmp_path):
    n_ds = 3
    dg = framing_catalogue()
    want, want_warns = expected(dg, n_ds)
    assert sum(sum(want[k].values()) for k in range(n_ds)) > 1000 and len(want_warns) > 50
    got, warns = run_router_framing(dg, n_ds, str(tmp_path))
    assert warns == want_warns
    assert got == want
