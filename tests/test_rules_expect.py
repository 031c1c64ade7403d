"""tests/rules_expect.py, the restatement the rules kernels are checked against, checked itself, and the C
validation against it (CPU only): bad rule sets, which rule wins, the edges of a match at the end of a line,
conservation on seeded batches, allow lists and the empty set."""
from __future__ import annotations

import errno

import numpy as np
import pytest

import rules_expect as E
from rules_expect import DROP, EXACT, KEEP, PREFIX

BAD_SETS = {
    "an empty pattern": [(b"", PREFIX, DROP)],
    "a 65-byte pattern": [(b"x" * 65, PREFIX, DROP)],
    "a ':' in a pattern": [(b"a:b", EXACT, DROP)],
    "a newline in a pattern": [(b"a\nb", PREFIX, DROP)],
    "duplicate rules": [(b"a.b", PREFIX, DROP), (b"c", EXACT, KEEP), (b"a.b", PREFIX, KEEP)],
    "257 rules": [(b"r%03d" % i, PREFIX, DROP) for i in range(257)],
    "4097 text bytes": [(b"%02d" % i + b"y" * 62, PREFIX, DROP) for i in range(64)] + [(b"z", EXACT, DROP)],
}

GOOD_SETS = {
    "no rules": [],
    "one byte": [(b"a", PREFIX, DROP)],
    "64 bytes": [(b"x" * 64, EXACT, DROP)],
    "EXACT and PREFIX of one text": [(b"a.b", PREFIX, DROP), (b"a.b", EXACT, KEEP)],
    "256 rules": [(b"r%03d" % i, PREFIX, DROP) for i in range(256)],
    "4096 text bytes": [(b"%02d" % i + b"y" * 62, PREFIX, DROP) for i in range(64)],
    "NUL and high bytes": [(b"\x00", PREFIX, DROP), (b"\xff\x80 #*", EXACT, DROP)],
}


@pytest.mark.parametrize("name", list(BAD_SETS))
def test_bad_sets_are_einval(pkg, name):
    rules = BAD_SETS[name]
    assert not E.check(rules)
    assert pkg.RuleSet(rules).check() == -errno.EINVAL


@pytest.mark.parametrize("name", list(GOOD_SETS))
def test_good_sets_pass(pkg, name):
    rules = GOOD_SETS[name]
    assert E.check(rules) and E.check(rules, DROP)
    assert pkg.RuleSet(rules).check() == 0 and pkg.RuleSet(rules, DROP).check() == 0


def test_bad_default_and_fields(pkg):
    assert not E.check([], 2) and pkg.RuleSet([], 2).check() == -errno.EINVAL
    assert pkg.RuleSet([(b"a", 2, DROP)]).check() == -errno.EINVAL and not E.check([(b"a", 2, DROP)])
    assert pkg.RuleSet([(b"a", PREFIX, 2)]).check() == -errno.EINVAL and not E.check([(b"a", PREFIX, 2)])
    assert pkg.lib().sr_rules_check(None) == -errno.EINVAL


def test_nested_prefixes_the_longest_wins():
    rules = [(b"a.", PREFIX, DROP), (b"a.b.c.", PREFIX, DROP), (b"a.b.", PREFIX, KEEP), (b"a.b.c.d", PREFIX, KEEP)]
    assert E.match(rules, b"a.x:1|c\n") == 0
    assert E.match(rules, b"a.b.x:1|c\n") == 2
    assert E.match(rules, b"a.b.c.x:1|c\n") == 1
    assert E.match(rules, b"a.b.c.d:1|c\n") == 3
    assert E.match(rules, b"b.a.:1|c\n") == 4
    assert E.match(list(reversed(rules)), b"a.b.c.x:1|c\n") == 2   # the same rule, wherever it stands


def test_exact_beats_prefix_on_the_equal_name_only():
    rules = [(b"svc.req", PREFIX, KEEP), (b"svc.req", EXACT, DROP)]
    assert E.match(rules, b"svc.req:1|c\n") == 1
    assert E.match(rules, b"svc.req.count:1|c\n") == 0
    assert E.match(rules, b"svc.reqs:1|c\n") == 0
    assert E.match(rules[1:], b"svc.req.count:1|c\n") == 1   # index 1 of a one-rule set: the default


def test_a_name_that_is_a_proper_prefix_of_a_pattern_matches_nothing():
    rules = [(b"svc.requests", PREFIX, DROP), (b"svc.requests", EXACT, DROP)]
    assert E.match(rules, b"svc.req:1|c\n") == 2
    assert E.match(rules, b"svc.request:12345|c\n") == 2


def test_the_pattern_at_the_end_of_the_line():
    """p = L - 1: a PREFIX matches, an EXACT cannot (no byte for the ':'); p = L - 2: the EXACT needs the ':'
    right before the last byte."""
    assert E.match([(b"abc", PREFIX, DROP)], b"abc\n") == 0          # p = 3 = L - 1
    assert E.match([(b"abc", PREFIX, DROP)], b"abc") == 1            # p = 3 = L: the last byte is never matched
    assert E.match([(b"abc", EXACT, DROP)], b"abc\n") == 1
    assert E.match([(b"abc", EXACT, DROP)], b"abc:") == 1            # p + 1 = L: the ':' would be the last byte
    assert E.match([(b"abc", EXACT, DROP)], b"abc:\n") == 0          # p = L - 2
    assert E.match([(b"abc", PREFIX, DROP)], b"abc:\n") == 0
    assert E.match([(b"abc", EXACT, DROP)], b"abcd\n") == 1
    assert E.match([(b"a", PREFIX, DROP)], b"a") == 1 and E.match([(b"a", PREFIX, DROP)], b"") == 1


def seeded(seed, count, n):
    rng = np.random.default_rng(seed)
    names = [b"debug.a", b"debug.b.c", b"app.req", b"app.req.count", b"app.r", b"sys.cpu", b"x"]
    lines = []
    for u, k, v in zip(rng.random(count), rng.integers(0, len(names), count), rng.integers(0, 3000, count)):
        if u < 0.85:
            lines.append(names[k] + b":%d|c" % v)
        elif u < 0.90:
            lines.append(b"ab")                      # invalid length
        elif u < 0.95:
            lines.append(b"debug.no colon here")     # invalid format: not subject
        else:
            lines.append(names[k] + b".%d:%d|ms" % (v, v))
    return E.records_of(lines, n)


RULES = [(b"debug.", PREFIX, DROP), (b"debug.b.", PREFIX, KEEP), (b"app.req", EXACT, DROP), (b"app.r", PREFIX, KEEP),
         (b"sys.cpu", EXACT, KEEP)]


@pytest.mark.parametrize("default", [KEEP, DROP])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_conservation(seed, default):
    data, recs, hashes = seeded(seed, 700, 3)
    res = E.apply(data, recs, hashes, 3, RULES, default)
    out, dropped, dbytes, subject = (int(x) for x in res.counts)
    assert out + dropped == len(recs)
    assert int(res.hits[:, 0].sum()) == subject == int((res.match != E.NOT_SUBJECT).sum())
    assert int(res.hits[:, 1].sum()) == int(recs["length"][res.match != E.NOT_SUBJECT].sum())
    assert dropped == sum(int(res.hits[i, 0]) for i, a in enumerate([a for _, _, a in RULES] + [default]) if a == DROP)
    assert dbytes == sum(int(res.hits[i, 1]) for i, a in enumerate([a for _, _, a in RULES] + [default]) if a == DROP)
    assert len(res.hashes_out) == out and 0 < dropped < subject < len(recs)
    # the records out are a subsequence of the records in
    it = iter(recs.tolist())
    assert all(any(r == x for x in it) for r in res.out.tolist())


def test_default_drop_is_an_allow_list():
    data, recs, hashes = E.records_of([b"app.req:1|c", b"other:1|c", b"ab", b"app.x:2|c"], 2)
    res = E.apply(data, recs, hashes, 2, [(b"app.", PREFIX, KEEP)], DROP)
    assert res.match.tolist() == [0, 1, E.NOT_SUBJECT, 0]
    assert res.out.tolist() == [recs[0].tolist(), recs[2].tolist(), recs[3].tolist()]   # the invalid line passes
    assert res.counts.tolist() == [3, 1, len(b"other:1|c\n"), 3]


@pytest.mark.parametrize("default", [KEEP, DROP])
def test_no_rules(default):
    data, recs, hashes = seeded(9, 300, 2)
    res = E.apply(data, recs, hashes, 2, [], default)
    subject = int((recs["route"] < 2).sum())
    assert res.hits.tolist() == [[subject, int(recs["length"][recs["route"] < 2].sum())]]
    assert int(res.counts[0]) == (len(recs) if default == KEEP else len(recs) - subject)


def test_records_that_are_not_subject():
    data = b"debug.a:1|c\n"
    recs = np.array([(0, 12, 0), (0, 12, 5), (0, 0, 0), (4, 12, 0), (0, 12, 0xFFFF)], E.RECORD_DTYPE)
    res = E.apply(data, recs, None, 2, [(b"debug.", PREFIX, DROP)])
    assert res.match.tolist() == [0, E.NOT_SUBJECT, E.NOT_SUBJECT, E.NOT_SUBJECT, E.NOT_SUBJECT]
    assert res.counts.tolist() == [4, 1, 12, 1] and res.hashes_out is None
