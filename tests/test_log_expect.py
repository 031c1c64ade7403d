"""tests/log_expect.py, the Python restatement of sr_format_log's output, pinned to the reference: for every
scripted session of tests/golden/router_*.json and every datagram of it, the helper over sr_oracle.route's
records and hashes under the current alive snapshot gives what sr_router_oracle.DataThread (pinned to the
compiled reference by tests/test_oracle_router.py) logs for that datagram, at log levels 0 and 3. And
SR_LOG_MAX_MSGS / SR_LOG_TEXT_CAPACITY hold on the worst-case streams. CPU only."""
from __future__ import annotations

import numpy as np
import pytest

import log_expect as L
from conftest import load_router_fixture, router_fixtures


@pytest.mark.parametrize("level", [0, 3])
@pytest.mark.parametrize("name", router_fixtures())
def test_helper_gives_the_reference_messages_per_datagram(oracle, name, level):
    import sr_router_oracle as R

    fx = load_router_fixture(name)
    n = fx["n"]
    alive = [0] * n
    seen = 0
    for e in fx["events"]:
        if e[0] == "alive":
            alive = [int(a) for a in e[1]]
            continue
        if e[0] != "dgram":
            continue
        dt = R.DataThread(n, fx["ds_hosts"], fx["ds_data_ports"], fx["ping_prefix"], fx["hostname"], fx["data_port"],
                          log_level=level)
        dt.set_alive(alive)
        dt.datagram(e[1])
        buf = oracle.frame(e[1])
        recs, hs, cnt = oracle.route(buf, n, alive)
        got = L.messages(buf, recs[:cnt], hs[:cnt], [len(buf)] if buf else [], n, level)
        assert got == dt.logs, (name, seen)
        seen += len(got)
    assert seen > 0 or level == 3


def test_whole_session_as_one_batch_with_ends(oracle):
    """Several datagrams in one batch, empty ones among them: the ends place every "got packet"."""
    import sr_router_oracle as R

    dgrams = [b"a:1|c", b"", b"bb:2|c\ncc:3|c\n", b"\n", b"", b"x\0y:1|c\nnocolon\n", b"\0\0\0", b"z" * 1500]
    n, alive = 3, [1, 0, 1]
    dt = R.DataThread(n, ["h"] * n, ["1"] * n, "p", "host", 1, log_level=0)
    dt.set_alive(alive)
    for d in dgrams:
        dt.datagram(d)
    framed = [oracle.frame(d) for d in dgrams]
    buf = b"".join(framed)
    ends = np.cumsum([len(f) for f in framed])
    recs, hs, cnt = oracle.route(buf, n, alive)
    assert L.messages(buf, recs[:cnt], hs[:cnt], ends, n, 0) == dt.logs
    assert L.messages(buf, recs[:cnt], None, ends, n, 3) == [m for m in dt.logs if m[0] >= 3]
    # without ends, and with ends that stop early, the "got packet" messages go and nothing else does
    no_got = [m for m in dt.logs if not m[1].startswith(b"udp_read_cb: got packet")]
    assert L.messages(buf, recs[:cnt], hs[:cnt], None, n, 0) == no_got
    few = L.messages(buf, recs[:cnt], hs[:cnt], ends[:3], n, 0)
    assert sum(m[1].startswith(b"udp_read_cb: got packet") for m in few) == 2 and len(few) == len(no_got) + 2


def test_wire_format():
    text, offs, lv = L.wire([(0, b"abc"), (3, b"defgh")], (b"T ", b"WW "), 0)
    assert text == b"T abc\nWW defgh\n" and offs.tolist() == [0, 6, 15] and lv.tolist() == [0, 3]
    text, offs, lv = L.wire([(0, b"abc"), (3, b"defgh")], (b"T ", b"WW "), 4)
    assert text == b"T ab\nWW d\n" and offs.tolist() == [0, 5, 10]


@pytest.mark.parametrize("k", [1, 2, 17, 4096])
@pytest.mark.parametrize("plen", [0, 35])
def test_capacity_holds_on_one_byte_lines(pkg, oracle, k, plen):
    """b"\\n" * k, as k one-byte datagrams and as datagrams of up to 4095 of them: the text's worst case."""
    buf = b"\n" * k
    recs, hs, cnt = oracle.route(buf, 4, None)
    for ends in (np.arange(1, k + 1), np.asarray(sorted({min(k, e) for e in range(4095, k + 4095, 4095)}))):
        text, offs, lv = L.expect(buf, recs[:cnt], hs[:cnt], ends, 4, 0, (b"t" * plen, b"w" * plen))
        assert lv.size <= pkg.log_max_msgs(k, len(ends)) == L.max_msgs(k, len(ends))
        assert len(text) <= pkg.log_text_capacity(k, len(ends), plen) == L.text_capacity(k, len(ends), plen)
    # one-byte datagrams meet the message bound exactly and press on the text bound
    text, offs, lv = L.expect(buf, recs[:cnt], hs[:cnt], np.arange(1, k + 1), 4, 0, (b"t" * plen, b"w" * plen))
    assert lv.size == pkg.log_max_msgs(k, k)
    assert len(text) > 0.9 * pkg.log_text_capacity(k, k, plen)


def test_capacity_holds_on_six_byte_lines_with_long_hashes(pkg, oracle):
    """6-byte valid lines whose hashes have 16 hex digits, 65533 shards: two messages per six bytes, the
    longest numbers."""
    lines, x = [], 0
    while len(lines) < 300:
        # the reference's `char c` is signed: a first name byte >= 0x80 wraps the hash to 2^64 - small
        line = bytes([0xF0 + (x & 15), 0x80 + ((x >> 4) & 0x7F), 0xFF]) + b":1\n"
        x += 1
        assert len(line) == 6
        h = oracle.hash_line(line)
        if h is not None and h >> 60:
            lines.append(line)
    buf = b"".join(lines)
    n = pkg.SR_MAX_DOWNSTREAMS
    recs, hs, cnt = oracle.route(buf, n, None)
    assert cnt == 300 and all(int(h) >> 60 for h in hs[:cnt]) and int(recs["route"][:cnt].max()) >= 10000
    for per in (1, 7, 300):
        ends = np.asarray([6 * min(300, j) for j in range(per, 300 + per, per)])
        for plen in (0, 256):
            text, offs, lv = L.expect(buf, recs[:cnt], hs[:cnt], ends, n, 0, (b"t" * plen, b"w" * plen))
            assert lv.size == 600 + len(ends) <= pkg.log_max_msgs(len(buf), len(ends))
            assert len(text) <= pkg.log_text_capacity(len(buf), len(ends), plen)
