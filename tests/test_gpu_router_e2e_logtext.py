"""GPU: statsd-router-mi355x with SR_DEVICE_LOG=1 at log_level 0 end to end over loopback: every batch's
log text is written on the GPU and reaches stdout in one write. Same harness as tests/test_gpu_router_e2e.py's
TRACE comparison: the data-path messages, whole and in order, are those of the reference's data thread (oracle
restatement; compared on each message's first 1900 bytes, which log_msg's 2048-byte buffer never cuts), the
packets are unchanged, and the reference executable (oracle/_ref/statsd-router), run the same way, gives the
same messages byte for byte, the cut ones included (a test of its own, skipped visibly where that executable
was not built, as in tests/test_gpu_router_e2e.py)."""
from __future__ import annotations

import os
import socket
import subprocess
import time
from collections import Counter

import pytest

from router_proc import OURS, REFERENCE, Router, config_text, free_ports
from test_gpu_router_e2e import PREFIX, SINK, catalogue

pytestmark = pytest.mark.gpu

DATA_PATH = (b"udp_read_cb:", b"process_data_line:", b"find_downstream:")


def _run(exe, datagrams, n_ds, tmp, env=None):
    base = free_ports(4 + 2 * n_ds)
    data_port, ctl, sink_base = base, base + 1, base + 4
    ds = [(sink_base + 2 * i, sink_base + 2 * i + 1) for i in range(n_ds)]
    dump = os.path.join(tmp, f"dump-{os.path.basename(exe)}.bin")
    sink = subprocess.Popen([SINK, str(sink_base), str(n_ds), "60", "3.0", dump], stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE)
    assert sink.stderr.readline().strip() == b"ready"
    r = Router(exe, config_text(data_port, ctl, ds, log_level=0, threads=1, flush=0.1, health=0.1, ping=1000.0,
                                prefix=PREFIX), tmp, env=env)
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
        for line in pkt.split(b"\n")[:-1]:
            if not line.startswith(PREFIX.encode()):
                got[d][line + b"\n"] += 1
    return got, [(lv, m) for lv, m in r.messages() if m.startswith(DATA_PATH)]


N_DS = 3


def _datagrams():
    dg = catalogue(seed=14)[:160]
    dg[40:40] = [b"J" * 4095, b"".join(b"long.%04d:1|c\n" % i for i in range(400))[:4095], b"", b"nul\0inside:1|c\nx\0y\n"]
    return dg


@pytest.fixture(scope="module")
def ours(tmp_path_factory):
    """(packets per downstream, data-path messages) of one run of the executable with SR_DEVICE_LOG=1."""
    return _run(OURS, _datagrams(), N_DS, str(tmp_path_factory.mktemp("ours")), env={"SR_DEVICE_LOG": "1"})


def test_device_log_prints_the_reference_trace(ours):
    import sr_router_oracle as RO

    n_ds, dg = N_DS, _datagrams()
    t = RO.DataThread(n_ds, ["127.0.0.1"] * n_ds, [str(9000 + i) for i in range(n_ds)], PREFIX, "h", 1, log_level=0)
    t.set_alive([1] * n_ds)
    for d in dg:
        t.datagram(d)
    t.flush_timer()
    want_pk = {i: Counter() for i in range(n_ds)}
    for s, pkts in t.packets.items():
        for p in pkts:
            for line in p.split(b"\n")[:-1]:
                want_pk[s][line + b"\n"] += 1
    names = {0: "TRACE", 3: "WARN"}
    want = [(names[lv], m[:1900]) for lv, m in t.logs]
    assert sum(lv == "TRACE" for lv, _ in want) > 2 * len(dg) and max(len(m) for _, m in t.logs) > 4000

    got_pk, m1 = ours
    assert got_pk == want_pk
    assert [(lv, m[:1900]) for lv, m in m1] == want


@pytest.mark.skipif(not os.path.exists(REFERENCE), reason="reference executable not built (make -C oracle ref)")
def test_device_log_matches_reference_executable(ours, tmp_path):
    got_pk, m1 = ours
    ref_pk, m2 = _run(REFERENCE, _datagrams(), N_DS, str(tmp_path))
    assert got_pk == ref_pk
    assert max(len(m) for _, m in m2) > 1950   # messages that log_msg's buffer cuts are in the comparison
    assert m1 == m2
