"""tests/validate_expect.py, the restatement of the line grammar, against the contract's own examples: accepted and
rejected families per reason, the precedence cases, the two corpora that must judge OK (the generator's traffic and
the router's ping lines) and conservation on seeded batches. CPU only, no library."""
from __future__ import annotations

import numpy as np
import pytest

import byte_streams
import validate_expect as E
from validate_expect import (EMPTY_NAME, NAME_BYTE, NO_COLON, NO_TYPE, OK, RATE, SECTION, TAGS, TYPE, VALUE)

ACCEPTED = [
    b"a:1|c", b"a:1|c\n", b"a:-1|c", b"a:1.5|c|@0.1", b"a:+1|g", b"a:-1.25|g", b"a:0|g|#t", b"a:12|ms|@1|#x:y,z",
    b"a:1|h", b"a:1|h|@0.5", b"a:1|d|@0.5|#a", b"a:x|s", b"a:a:b|s", b"a:" + b"v" * 64 + b"|s", b"a:1|s|#t",
    b"a:" + b"9" * 20 + b"." + b"9" * 20 + b"|c", b"!~{}:1|c", b"a:1|c|#" + b"t" * 1400, b"a:1|c|#a:b,c:d",
]
REJECTED = {
    NO_COLON: [b"abc", b"abc\n", b"\n", b"a|c", b"a\n", b"1|c|@1"],
    EMPTY_NAME: [b":1|c", b":", b":\n", b"::1|c"],
    NAME_BYTE: [b"a b:1|c", b"a|b:1|c", b"a\x00:1|c", b"\xff:1|c", b"a\nb:1|c", b"\x7f:1|c", b" :1|c"],
    NO_TYPE: [b"a:1", b"a:", b"a:\n", b"a:x", b"a:1:2", b"a:@1#t"],
    TYPE: [b"a:1|", b"a:1|q", b"a:1|C", b"a:1|cc", b"a:1|m", b"a:1|msx", b"a:1|c |@1", b"a:x|q", b"a:1||c", b"a:1|\n|c",
           b"a:1|c\n\n"],
    VALUE: [b"a:|c", b"a:x|c", b"a:+1|c", b"a:--1|c", b"a:1.|c", b"a:.5|c", b"a:1.2.3|c", b"a:1e5|c", b"a:-1|ms", b"a:+1|h",
            b"a:-1|d", b"a:" + b"1" * 21 + b"|c", b"a:1." + b"1" * 21 + b"|g", b"a:|s", b"a:" + b"v" * 65 + b"|s",
            b"a:a b|s", b"a:\x00|s", b"a:1 |c", b"a:1\n|c", b"a: 1|c", b"a:-|c", b"a:+|g"],
    SECTION: [b"a:1|c|", b"a:1|c|x", b"a:1|c|@1|@1", b"a:1|c|#t|@1", b"a:1|c|#t|#u", b"a:1|c|#t|", b"a:1|c|@1|", b"a:1|c||#t",
              b"a:1|c|@1||", b"a:1|g|x"],
    RATE: [b"a:1|c|@", b"a:1|c|@x", b"a:1|c|@-1", b"a:1|c|@+1", b"a:1|c|@1.", b"a:1|g|@0.5", b"a:1|s|@1", b"a:1|c|@|#t",
           b"a:1|c|@" + b"1" * 21, b"a:1|c|@0.5 ", b"a:1|g|@x|#t"],
    TAGS: [b"a:1|c|#", b"a:1|c|#\n", b"a:1|c|# ", b"a:1|c|#a b", b"a:1|c|#a\x00", b"a:1|c|#\xc3\xa9", b"a:1|c|@1|#", b"a:1|c|#|",
           b"a:1|c|#a\nb|@1", b"a:1|c|#t\n\n"],
}


@pytest.mark.parametrize("line", ACCEPTED)
def test_accepted(line):
    assert E.judge(line) == OK


@pytest.mark.parametrize("reason", sorted(REJECTED))
def test_rejected_families(reason):
    for line in REJECTED[reason]:
        assert E.judge(line) == reason, line
        if not line.endswith(b"\n"):
            assert E.judge(line + b"\n") == reason, line


def test_precedence():
    assert E.judge(b"a:x") == NO_TYPE            # not VALUE
    assert E.judge(b"a:x|q") == TYPE             # the type comes before the value
    assert E.judge(b"a:1|g|@0.5") == RATE
    assert E.judge(b"a:1|c|#t|@1") == SECTION
    assert E.judge(b"a:1|c|@1|@1") == SECTION
    assert E.judge(b"a b:x") == NAME_BYTE        # the name before the fields
    assert E.judge(b"a:1|c|@x|#") == RATE        # fields from left to right
    assert E.judge(b"a:1|c|#|x") == TAGS


def test_accept_types():
    assert E.judge(b"a:1|ms", E.TYPE_BITS[b"c"]) == TYPE and E.judge(b"a:1|c", E.TYPE_BITS[b"c"]) == OK
    assert E.judge(b"a:x|ms", E.TYPE_BITS[b"c"]) == TYPE
    assert E.judge(b"a:x|s", E.TYPES_ALL & ~16) == TYPE


def test_configurations():
    assert E.check(0, E.TYPES_ALL) and E.check(E.DROP_ALL, 1) and E.check(1 << 9, 32)
    assert not E.check(1, E.TYPES_ALL) and not E.check(1 << 10, E.TYPES_ALL) and not E.check(0, 0) and not E.check(0, 64)
    assert E.parse_spec("count") == (0, 63) and E.parse_spec("drop") == (0x3FE, 63)
    assert E.parse_spec("value,tags") == ((1 << VALUE) | (1 << TAGS), 63)
    for bad in ("", "ok", "value,", ",value", "Value", "drop,count", "value tags"):
        assert E.parse_spec(bad) is None, bad


def test_the_generators_traffic_is_ok():
    """tests/byte_streams.py lines of the name:1|c kind whose names lie inside NB."""
    rng = np.random.default_rng(5)
    nb = set(range(0x21, 0x7F)) - set(b":|")
    seen = 0
    for n in byte_streams.NAME_LENGTHS:
        tail = byte_streams.name_tail(n)
        for _ in range(20):
            name = bytes(b if b in nb else 0x61 + b % 26 for b in byte_streams.uniform_name(rng, n))
            assert E.judge(name + tail) == (OK if tail == b":1|c\n" else NO_TYPE)
            seen += tail == b":1|c\n"
    assert seen >= 20 * (len(byte_streams.NAME_LENGTHS) - 1)


def test_the_routers_ping_lines_are_ok():
    for line in (b"statsd-router.host-8125.ds1-8125.connections:1|c\n", b"statsd-router.ds1-8125.connections:1|c\n",
                 b"statsd-router.alive.downstreams:0|g\n", b"p.h-1.alive:%d|g\n" % 12, b"x.traffic:123456|c\n"):
        assert E.judge(line) == OK, line


def test_conservation_on_seeded_batches():
    rng = np.random.default_rng(11)
    pool = ACCEPTED + [x for v in REJECTED.values() for x in v]
    pool = [x.rstrip(b"\n") for x in pool if b"\n" not in x.rstrip(b"\n") and len(x.rstrip(b"\n")) >= 1]
    for seed in range(4):
        lines = [pool[k] for k in rng.integers(0, len(pool), 500)]
        data, recs, hashes = E.records_of(lines, 4)
        for mask in (0, E.DROP_ALL, 1 << VALUE, (1 << NO_COLON) | (1 << TAGS)):
            res = E.apply(data, recs, hashes, 4, mask)
            assert int(res.counts[0] + res.counts[1]) == len(recs) and len(res.out) == int(res.counts[0])
            assert int(res.hits[:, 0].sum()) == int(res.counts[3])
            dropped = sum(int(res.hits[r, 0]) for r in range(E.REASONS) if mask >> r & 1)
            assert dropped == int(res.counts[1])
            assert int(res.counts[2]) == sum(int(res.hits[r, 1]) for r in range(E.REASONS) if mask >> r & 1)
            assert len(res.hashes_out) == len(res.out)
            if mask == 0:
                assert np.array_equal(res.out, recs)
