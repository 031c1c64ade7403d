"""tests/coalesce_expect.py, the restatement the coalescing kernels are checked against, checked itself (CPU
only): the grammar's accepted and rejected lines, conservation on seeded random batches, and the length and
append bounds of include/sr_route.h on their worst families."""
from __future__ import annotations

import re

import numpy as np
import pytest

import coalesce_expect as E

ACCEPTED = [
    (b"a:1|c\n", 1, 1),                                   # the shortest line
    (b"test.counter:1|c\n", 12, 1),
    (b"x.y:0|c\n", 3, 0),
    (b"x.y:-0|c\n", 3, 0),                                # "-0" is accepted
    (b"x.y:007|c\n", 3, 7),                               # leading zeros are accepted
    (b"x.y:999999999|c\n", 3, 999999999),                 # nine digits
    (b"x.y:-999999999|c\n", 3, -999999999),
    (b"x.y:000000000|c\n", 3, 0),
    (b"n\x00\xff\x80 \t|c:12|c\n", 8, 12),                 # NUL, high bytes, blanks and "|c" inside a name
    (b"a\nb:3|c\n", 3, 3),                                # a name byte is anything but ':'
    (b"n" * 1425 + b":5|c\n", 1425, 5),                   # the longest name
    (b"n" * 1425 + b":-999999999|c\n", 1425, -999999999),
]

REJECTED = [
    b"a:1|c",                                             # no '\n'
    b":1|c\n",                                            # an empty name (and five bytes)
    b":12|c\n",                                           # an empty name in six bytes
    b"x.y:+1|c\n",                                        # a '+'
    b"x.y:1234567890|c\n",                                # a tenth digit
    b"x.y:-1234567890|c\n",
    b"x.y:1|c|@0.1\n",                                    # a sample rate
    b"x.y:1|ms\n",                                        # another type
    b"x.y:1|g\n",
    b"x.y:1|C\n",
    b"x.y:1.5|c\n",                                       # a float
    b"x.y:1e3|c\n",
    b"x.y:|c\n",                                          # an empty value
    b"x.y:-|c\n",
    b"x.y:--1|c\n",
    b"x.y:1-|c\n",
    b"x.y:1|c|#tag:v\n",                                  # tags
    b"x.y:1|c\r\n",                                       # a '\r'
    b"x.y:1|c \n",
    b"x.y: 1|c\n",
    b"x.y:1 |c\n",
    b"x:y:1|c\n",                                         # the first ':' is not the one before the number
    b"x.y:1|c\n\n",
    b"x.y:1|c\nz:1|c\n",                                  # two lines are not one
    b"no colon in this line|c\n",
    b"x.y:1\n",
    b"x.y:1|\n",
    b"x.y:1c\n",
    b"n" * 1426 + b":5|c\n",                              # one name byte too many
    b"n" * 1445 + b":5|c\n",                              # 1450 bytes: not a valid line at all
    b"",
    b"\n",
]


@pytest.mark.parametrize("line,k,v", ACCEPTED, ids=[str(i) for i in range(len(ACCEPTED))])
def test_grammar_accepts(line, k, v):
    assert E.parse(line) == (k, v)


@pytest.mark.parametrize("line", REJECTED, ids=[str(i) for i in range(len(REJECTED))])
def test_grammar_rejects(line):
    assert E.parse(line) is None


def test_dec_and_merged_line():
    assert E.merged_line(b"a", 0) == b"a:0|c\n" and E.merged_line(b"a", -5) == b"a:-5|c\n"
    assert E.merged_line(b"a.b", 10 ** 18) == b"a.b:1000000000000000000|c\n"
    assert E.parse(E.merged_line(b"a.b", 999999999)) == (3, 999999999)
    assert len(E.merged_line(b"n" * E.NAME_MAX, -(1 << 62))) == E.MAX_LINE   # 1425 + 1 + 20 + 3


def random_batch(seed, count, n, pool=40):
    rng = np.random.default_rng(seed)
    lines = []
    for u, k, v in zip(rng.random(count), rng.integers(0, pool, count), rng.integers(-2000, 2000, count)):
        if u < 0.35:
            lines.append(b"hot.name:%d|c" % v)
        elif u < 0.70:
            lines.append(b"svc.req.%d:%d|c" % (k, v))
        elif u < 0.78:
            lines.append(b"svc.req.%d:%d|ms" % (k, abs(v)))
        elif u < 0.84:
            lines.append(b"svc.req.%d:%d|c|@0.5" % (k, abs(v)))
        elif u < 0.88:
            lines.append(b"ab")                          # invalid length
        elif u < 0.92:
            lines.append(b"no colon in this line")       # invalid format
        else:
            lines.append(b"g.%d:%d.5|g" % (k, abs(v)))
    return E.records_of(lines, n)


def routed_lines(data, res, recs):
    return [(int(r["route"]), E.line_of(data, res, r)) for r in recs]


@pytest.mark.parametrize("seed,slots", [(1, 16), (2, 16), (3, 64), (4, E.DEFAULT_SLOTS), (5, 16)])
def test_conservation_on_random_batches(seed, slots):
    n = 5
    data, recs, hashes = random_batch(seed, 700, n)
    res = E.coalesce(data, recs, hashes, n, slots)
    before = E.ledger((int(r["route"]), data[int(r["offset"]):int(r["offset"]) + int(r["length"])]) for r in recs)
    after = E.ledger(routed_lines(data, res, res.out))
    assert before[0] == after[0]                          # per (route, name): the sums, read back from the text
    assert before[1] == after[1]                          # every other line unchanged and in order
    c = res.counts.tolist()
    assert c[0] == len(res.out) and c[0] + c[1] == len(recs) and c[3] == len(res.text)
    assert c[2] > 0 and c[1] >= c[2]
    assert len(res.text) <= len(data) and res.complete
    merged = [r for r in res.out if int(r["offset"]) >= len(data)]
    assert len(merged) == c[2] and all(E.MIN_LINE <= int(r["length"]) <= E.MAX_LINE for r in merged)


def test_collisions_leave_lines_unmerged_but_never_wrong():
    """Two names on one slot (made-up hashes): the later name keeps all its lines; same hash, other bytes: too."""
    lines = [b"first:1|c", b"second:2|c", b"first:3|c", b"second:4|c", b"third:5|c", b"third:6|c"]
    data, recs, _ = E.records_of(lines, 1)
    h = [E.fmix64_inverse(16 * 5 + 3), E.fmix64_inverse(16 * 9 + 3), 0, 0, 77, 77]
    h[2], h[3] = h[0], h[1]
    res = E.coalesce(data, recs, np.array(h, np.uint64), 1, 16)
    got = [E.line_of(data, res, r) for r in res.out]
    assert got == [b"first:4|c\n", b"second:2|c\n", b"second:4|c\n", b"third:11|c\n"]
    assert res.counts.tolist() == [4, 2, 2, len(b"first:4|c\nthird:11|c\n")]
    same = E.coalesce(data, recs, np.zeros(6, np.uint64), 1, 16)     # one hash for three names
    assert [E.line_of(data, same, r) for r in same.out] == \
        [b"first:4|c\n", b"second:2|c\n", b"second:4|c\n", b"third:5|c\n", b"third:6|c\n"]


WORST = {
    "two nine-digit negatives": [b"%s:-999999999|c" % (b"m%03d" % (i // 2)) for i in range(400)],
    "k = 1": [bytes([65 + i // 2 % 26]) + b":9|c" for i in range(400)],
    "k = 1425": [bytes([65 + i // 2]) * 1425 + b":-999999999|c" for i in range(8)],
    "k = 1 and 9 + 1": [b"a:9|c", b"a:1|c"],              # 12 bytes in, a:10|c\n out: 7
}


@pytest.mark.parametrize("family", list(WORST))
def test_bounds_on_the_worst_families(family):
    data, recs, hashes = E.records_of(WORST[family], 3)
    res = E.coalesce(data, recs, hashes, 3, E.MAX_SLOTS)   # no two of these names share a slot there
    assert int(res.counts[2]) == len(set(WORST[family][i].split(b":")[0] for i in range(len(recs))))
    assert int(res.counts[3]) <= len(data) == E.append_capacity(len(data))
    for r in res.out:
        assert int(r["offset"]) >= len(data) and E.MIN_LINE <= int(r["length"]) <= E.MAX_LINE
        assert re.fullmatch(rb"[^:]+:-?[1-9][0-9]*\|c\n", E.line_of(data, res, r))   # (a sum may have ten digits)


def test_a_name_of_1426_bytes_stays_unmerged():
    data, recs, hashes = E.records_of([b"n" * 1426 + b":1|c"] * 2 + [b"n" * 1425 + b":1|c"] * 2, 2)
    res = E.coalesce(data, recs, hashes, 2, 16)
    assert res.counts.tolist() == [3, 1, 1, 1425 + 5]
    assert [int(r["length"]) for r in res.out] == [1431, 1431, 1430]


def test_merged_line_is_never_longer_than_its_group():
    """1 + digits(c) <= 5 (c - 1) for c >= 2, and the sum of c values of d digits has at most d + digits(c)."""
    for c in list(range(2, 2000)) + [10 ** 6, 10 ** 9, 2 ** 30]:
        assert 1 + len(str(c)) <= 5 * (c - 1)
        for d in (1, 5, 9):
            assert len(str(c * (10 ** d - 1))) <= d + len(str(c))
    assert (1 << 30) // 6 * 999999999 < 1 << 60


def test_records_outside_the_batch_and_route_codes_pass_through():
    data, recs, hashes = E.records_of([b"a.b:1|c", b"a.b:2|c", b"a.b:3|c", b"a.b:4|c"], 2)
    recs = recs.copy()
    recs[1]["offset"] = len(data) - 3                     # runs past the end
    recs[2]["route"] = 0xFFFF                             # all dead
    res = E.coalesce(data, recs, hashes, 2, 16)
    assert res.counts.tolist() == [3, 1, 1, 8]
    assert E.line_of(data, res, res.out[0]) == b"a.b:5|c\n"
    assert res.out[1] == recs[1] and res.out[2] == recs[2]
    cut = E.coalesce(data, recs, hashes, 2, 16, append_cap=7)
    assert cut.written == b"a.b:5|c" and not cut.complete and np.array_equal(cut.out, res.out)
    few = E.coalesce(data, recs, hashes, 2, 16, n_records=1 << 40, max_records=1)
    assert few.counts.tolist() == [1, 0, 0, 0] and few.out[0] == recs[0]
