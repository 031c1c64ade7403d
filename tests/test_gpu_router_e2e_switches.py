"""GPU: statsd-router-mi355x with its SR_* switches together, end to end over loopback (the harness of
tests/test_gpu_router_e2e_logtext.py and tests/test_gpu_router_e2e_coalesce.py: the sink answers the downstreams'
health checks and dumps every packet).

Run 1, the switches that must not change the output, all on: SR_DEVICE_FRAMING=1 SR_DEVICE_LOG=1 SR_NAME_STATS=1 at
log_level 0. Packets and data-path messages are those of the reference's data thread (the oracle's restatement, and
the reference executable where it was built).

Run 2, all five: SR_COALESCE=1 and SR_NAME_RULES=<file> too, with hostile traffic and a ping every second. Which
datagrams share a batch depends on how recvmmsg groups them, so only what every grouping conserves is checked: no
dropped name arrives, the sum per name at each downstream and the multiset of the lines that are no plain counters
are those of the kept lines, nothing is logged at ERROR; and the per-ping lines report the dropped lines and, in the
name_stats line, the coalesced ones."""
from __future__ import annotations

import os
import re
import socket
import subprocess
import time
from collections import Counter

import pytest

import coalesce_expect as CE
import rules_expect as E
import switch_model as M
from router_proc import OURS, REFERENCE, Router, config_text, free_ports
from test_gpu_router_e2e import PREFIX, SINK
from test_gpu_router_e2e_logtext import N_DS, _datagrams, _run

pytestmark = pytest.mark.gpu

QUIET = {"SR_DEVICE_FRAMING": "1", "SR_DEVICE_LOG": "1", "SR_NAME_STATS": "1"}
FILE = b"# muted\ndrop debug.*\nkeep debug.keep.*\ndrop svc.req.7\ndrop host.hot\n"
RULES = M.RULES[:4]   # the rule file's: its format is text, the model's fifth pattern is not


# ---- run 1 ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quiet(tmp_path_factory):
    """(packets per downstream, data-path messages) of one run with the three switches that change no output."""
    return _run(OURS, _datagrams(), N_DS, str(tmp_path_factory.mktemp("quiet")), env=QUIET)


def test_framing_log_and_statistics_together_change_nothing(quiet):
    import sr_router_oracle as RO

    dg = _datagrams()
    t = RO.DataThread(N_DS, ["127.0.0.1"] * N_DS, [str(9000 + i) for i in range(N_DS)], PREFIX, "h", 1, log_level=0)
    t.set_alive([1] * N_DS)
    for d in dg:
        t.datagram(d)
    t.flush_timer()
    want_pk = {i: Counter() for i in range(N_DS)}
    for s, pkts in t.packets.items():
        for p in pkts:
            for line in p.split(b"\n")[:-1]:
                want_pk[s][line + b"\n"] += 1
    names = {0: "TRACE", 3: "WARN"}
    want = [(names[lv], m[:1900]) for lv, m in t.logs]
    assert sum(lv == "TRACE" for lv, _ in want) > 2 * len(dg)
    got_pk, msgs = quiet
    assert got_pk == want_pk
    assert [(lv, m[:1900]) for lv, m in msgs] == want


@pytest.mark.skipif(not os.path.exists(REFERENCE), reason="reference executable not built (make -C oracle ref)")
def test_framing_log_and_statistics_together_match_the_reference_executable(quiet, tmp_path):
    got_pk, m1 = quiet
    ref_pk, m2 = _run(REFERENCE, _datagrams(), N_DS, str(tmp_path))
    assert got_pk == ref_pk
    assert m1 == m2


# ---- run 2 ------------------------------------------------------------------------------------------------------
def test_all_five_switches_conserve_the_kept_lines(tmp_path, oracle):
    tmp = str(tmp_path)
    dgrams = M.datagrams(M.hostile_traffic(77, 3000), 77)
    base = free_ports(4 + 2 * N_DS)
    data_port, ctl, sink_base = base, base + 1, base + 4
    ds = [(sink_base + 2 * i, sink_base + 2 * i + 1) for i in range(N_DS)]
    dump, path = os.path.join(tmp, "dump.bin"), os.path.join(tmp, "rules.txt")
    with open(path, "wb") as f:
        f.write(FILE)
    # the pings keep the sink busy: it ends 1.5 s after the router was stopped
    sink = subprocess.Popen([SINK, str(sink_base), str(N_DS), "60", "1.5", dump], stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE)
    assert sink.stderr.readline().strip() == b"ready"
    r = Router(OURS, config_text(data_port, ctl, ds, log_level=1, threads=1, flush=0.1, health=0.1, ping=1.0,
                                 prefix=PREFIX), tmp, env=dict(QUIET, SR_COALESCE="1", SR_NAME_RULES=path))
    stats_line = re.compile(rb"name_stats: lines=\d+ .* coalesced=(\d+)/(\d+)$")
    try:
        for i in range(N_DS):
            assert r.wait_for(lambda lv, m, i=i: m == b"ds_health_read_cb downstream %d is up" % i, 20), r.raw[-20:]
        time.sleep(0.3)   # the data thread has seen the alive bits
        s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        for d in dgrams:
            s.sendto(d, ("127.0.0.1", data_port))
            time.sleep(0.0005)
        s.close()
        merged = lambda lv, m: lv == "INFO" and (stats_line.search(m) or [0, b"0"])[1] != b"0"
        assert r.wait_for(merged, 8), [m for lv, m in r.lines if b"name_stats" in m]
        assert r.wait_for(lambda lv, m: lv == "INFO" and m.startswith(b"name_rules: dropped lines="), 8), \
            [m for lv, m in r.lines if b"name_rules" in m]
        time.sleep(0.3)   # a flush interval: the last pending packets are out
    finally:
        r.stop()
        try:
            sink.communicate(timeout=30)
        finally:
            if sink.poll() is None:
                sink.kill()
    assert ("INFO", b"main: name_rules: 4 rules, default keep") in r.lines
    assert [m for lv, m in r.lines if lv == "ERROR"] == []
    got = []
    with open(dump, "rb") as f:
        blob = f.read()
    i = 0
    while i < len(blob):
        d, l = int.from_bytes(blob[i:i + 2], "little"), int.from_bytes(blob[i + 2:i + 4], "little")
        pkt = blob[i + 4:i + 4 + l]
        i += 4 + l
        assert len(pkt) <= 1450 and pkt.endswith(b"\n")
        got += [(d, line + b"\n") for line in pkt.split(b"\n")[:-1] if not line.startswith(PREFIX.encode())]
    # what was sent: every valid line at its shard, less what the rule file drops
    kept, dropped = [], 0
    actions = [a for _, _, a in RULES] + [E.KEEP]
    for d in dgrams:
        framed = oracle.frame(d)
        recs, _, _ = oracle.route(framed, N_DS, None)
        for rec in recs:
            line = framed[int(rec["offset"]): int(rec["offset"]) + int(rec["length"])]
            if int(rec["route"]) >= N_DS:
                continue
            if actions[E.match(RULES, line)] == E.KEEP:
                kept.append((int(rec["route"]), line))
            else:
                dropped += 1
    assert dropped > 500 and len(kept) > 1000
    assert not any(l.startswith((b"debug.t", b"host.hot:", b"svc.req.7:")) for _, l in got)
    want_sums, want_rest = CE.ledger(kept)
    got_sums, got_rest = CE.ledger(got)
    assert got_sums == want_sums
    assert Counter(got_rest) == Counter(want_rest)
    assert sum(CE.parse(l) is not None for _, l in got) < sum(CE.parse(l) is not None for _, l in kept)   # it did merge
