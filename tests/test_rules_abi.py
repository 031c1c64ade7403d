"""The name rules' entry points: declared, listed, exported, the structures and constants the same in C and Python,
argument errors that need no device, sr_rules_match against tests/rules_expect.py (every single-byte mutation of a
few lines, 10,000 seeded random lines against random rule sets that share prefixes) and sr_rules_parse_text on
accepted and rejected files. CPU only: needs the built libraries, calls no GPU code."""
from __future__ import annotations

import ctypes
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import rules_expect as E
from conftest import REPO
from rules_expect import DROP, EXACT, KEEP, PREFIX
from test_abi import _exported, declared_functions

NEW = {"sr_rules_open", "sr_rules_close", "sr_rules", "sr_rules_read", "sr_rules_reset", "sr_rules_check",
       "sr_rules_match", "sr_rules_parse_text", "sr_rules_free", "sr_set_name_rules", "sr_route_pack_rules"}


def test_new_functions_declared_listed_exported(pkg):
    assert NEW <= declared_functions()
    assert NEW <= set(pkg.ABI_FUNCTIONS)
    assert NEW <= _exported(pkg.ROUTE_LIB)
    lib = pkg.lib()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name
    for name in ("rules_open", "rules_close", "rules", "rules_batches", "rules_read", "rules_reset", "set_name_rules",
                 "route_pack_rules"):
        assert callable(getattr(pkg.Router, name)), name


def test_structures_and_constants_match_c(pkg, tmp_path):
    structs = {"sr_rule": pkg.SrRule, "sr_rules_config": pkg.SrRulesConfig, "sr_rules_batch": pkg.SrRulesBatch,
               "sr_rule_hits": pkg.SrRuleHits}
    consts = ["SR_RULES_MAX", "SR_RULES_PATTERN_MAX", "SR_RULES_TEXT_MAX", "SR_RULES_NOT_SUBJECT", "SR_RULE_PREFIX",
              "SR_RULE_EXACT", "SR_RULE_DROP", "SR_RULE_KEEP"]
    body, want = "", []
    for cname, py in structs.items():
        body += f'  printf(" %zu", sizeof({cname}));\n'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'  printf(" %zu", offsetof({cname}, {f}));\n'
            want.append(getattr(py, f).offset)
    for c in consts:
        body += f'  printf(" %lu", (unsigned long){c});\n'
        want.append(getattr(pkg, c))
    src = tmp_path / "rules.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sr_route.h"\nint main(void) {\n' + body
                   + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "rules"
    subprocess.run([os.environ.get("CC", "cc"), "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert out == want
    assert (E.RULES_MAX, E.PATTERN_MAX, E.TEXT_MAX, E.NOT_SUBJECT, E.PREFIX, E.EXACT, E.DROP, E.KEEP) == tuple(out[-8:])


def test_tile_constant_is_the_kernels(pkg):
    src = open(os.path.join(REPO, "statsd-router_amd", "csrc", "rules_kernel.hpp")).read()
    block = int(re.search(r"constexpr int kRulesBlock = (\d+);", src).group(1))
    assert re.search(r"constexpr int kRulesTile = kRulesBlock;", src)
    assert pkg.RULES_TILE == block


def test_argument_errors_need_no_device(pkg):
    lib = pkg.lib()
    rs = pkg.RuleSet([(b"a", PREFIX, DROP)])
    b = (pkg.SrRulesBatch * 1)()
    h = (pkg.SrRuleHits * 2)()
    c4 = (ctypes.c_uint64 * 4)()
    assert lib.sr_rules_open(None, rs.ref()) == -errno.EINVAL
    assert lib.sr_rules_close(None) == -errno.EINVAL
    assert lib.sr_rules(None, b, 1) == -errno.EINVAL
    assert lib.sr_rules_read(None, h, 2) == -errno.EINVAL
    assert lib.sr_rules_reset(None) == -errno.EINVAL
    assert lib.sr_set_name_rules(None, rs.ref()) == -errno.EINVAL
    assert lib.sr_route_pack_rules(None, 0, c4) == -errno.EINVAL
    assert lib.sr_rules_match(None, b"a:1|c\n", 6) == -errno.EINVAL
    assert lib.sr_rules_match(rs.ref(), None, 6) == -errno.EINVAL
    assert lib.sr_rules_match(rs.ref(), None, 0) == 1          # no bytes: the default
    assert lib.sr_rules_parse_text(b"drop a\n", 7, None, None) == -errno.EINVAL
    lib.sr_rules_free(None)


SETS = [
    [],
    [(b"a", PREFIX, DROP)],
    [(b"svc.req", PREFIX, KEEP), (b"svc.req", EXACT, DROP), (b"svc.", PREFIX, DROP), (b"svc.req.count", EXACT, KEEP)],
    [(b"abcdefgh", PREFIX, DROP), (b"abcdefghi", EXACT, DROP), (b"abcdefgh1234567", PREFIX, KEEP),
     (b"abcdefgh12345678", PREFIX, DROP), (b"abcdefgh123456789", EXACT, KEEP)],
    [(b"n\x00", PREFIX, DROP), (b"n", EXACT, KEEP), (b"n\x00\x00", EXACT, DROP), (b"n\x00\xff", PREFIX, KEEP),
     (b"\xff", PREFIX, DROP)],
    [(b"x" * 64, EXACT, DROP), (b"x" * 64, PREFIX, KEEP), (b"x" * 63, PREFIX, DROP), (b"x" * 17, EXACT, DROP)],
]
LINES = [b"svc.req:1|c\n", b"svc.req.count:12|ms\n", b"abcdefgh123456789:5|g\n", b"n\x00\x00:1|c\n", b"n:1|c\n",
         b"x" * 64 + b":1|c\n", b"x" * 17 + b":1\n", b"a\n"]


def test_match_agrees_with_the_restatement_on_mutations(pkg):
    """Every single-byte change, deletion and insertion of a few lines, from a small alphabet, and every prefix
    of each line."""
    alphabet = b":\n.ax1\x00\xff"
    n = 0
    for rules in SETS:
        rs = pkg.RuleSet(rules)
        assert rs.check() == 0
        for s in LINES:
            cases = {s[:k] for k in range(len(s) + 1)}
            for at in range(len(s) + 1):
                for ch in alphabet:
                    cases.update((s[:at] + bytes([ch]) + s[at:], s[:at] + bytes([ch]) + s[at + 1:], s[:at] + s[at + 1:]))
            for line in cases:
                assert rs.match(line) == E.match(rules, line), (rules, line)
                n += 1
    assert n > 15000   # the cases are sets: equal mutations count once


def random_set(rng, n_rules):
    """Rules that share prefixes: texts grown from one another over a tiny alphabet, NUL included."""
    alphabet = np.frombuffer(b"ab.\x00", np.uint8)
    texts = [bytes(rng.choice(alphabet, int(rng.integers(1, 4))))]
    rules, seen = [], set()
    while len(rules) < n_rules:
        base = texts[int(rng.integers(0, len(texts)))]
        t = (base + bytes(rng.choice(alphabet, int(rng.integers(0, 12)))))[:64 if n_rules <= 64 else 20]   # within 4096 bytes
        kind = int(rng.integers(0, 2))
        if (kind, t) in seen:
            continue
        seen.add((kind, t))
        texts.append(t)
        rules.append((t, kind, int(rng.integers(0, 2))))
    return rules, texts


def test_match_agrees_with_the_restatement_on_random_lines(pkg):
    rng = np.random.default_rng(11)
    alphabet = np.frombuffer(b"ab.\x00:", np.uint8)
    n = hits = 0
    for n_rules in (1, 3, 17, 64, 200):
        rules, texts = random_set(rng, n_rules)
        assert E.check(rules)
        rs = pkg.RuleSet(rules)
        for _ in range(2000):
            t = texts[int(rng.integers(0, len(texts)))]
            cut = int(rng.integers(0, len(t) + 1))
            line = t[:cut] + bytes(rng.choice(alphabet, int(rng.integers(0, 10)))) + (b"\n" if rng.random() < 0.8 else b"")
            want = E.match(rules, line)
            assert rs.match(line) == want, (rules, line)
            n += 1
            hits += want != len(rules)
    assert n == 10000 and hits > 2000


GOOD_FILE = b"""# a comment
drop debug.*

keep debug.keep.*
drop app.x
keep  two spaces *
drop we#ird name\r
default drop
"""


def test_parse_text_accepts(pkg):
    rs = pkg.rules_parse_text(GOOD_FILE)
    assert rs.rules == [(b"debug.", PREFIX, DROP), (b"debug.keep.", PREFIX, KEEP), (b"app.x", EXACT, DROP),
                        (b" two spaces ", PREFIX, KEEP), (b"we#ird name\r", EXACT, DROP)]
    assert rs.default_action == DROP and rs.check() == 0
    assert pkg.rules_parse_text(b"").rules == [] and pkg.rules_parse_text(b"").default_action == KEEP
    assert pkg.rules_parse_text(b"keep a").rules == [(b"a", EXACT, KEEP)]              # no '\n' at the end
    assert pkg.rules_parse_text(b"drop " + b"x" * 64 + b"*\n").rules == [(b"x" * 64, PREFIX, DROP)]
    assert len(pkg.rules_parse_text(b"".join(b"drop r%03d\n" % i for i in range(256)))) == 256


BAD_FILES = [
    (b"drop a\nmute b\n", 2),                                  # an unknown word
    (b"drop\n", 1),                                            # no pattern
    (b"drop \n", 1),                                           # an empty pattern
    (b"# x\n\ndrop *\n", 3),                                   # an empty prefix
    (b"drop a:b\n", 1),                                        # a ':' in a pattern
    (b"keep a\ndrop b*\nkeep a\n", 3),                         # a duplicate: the second of the two
    (b"drop " + b"x" * 65 + b"\n", 1),                         # 65 bytes
    (b"drop " + b"x" * 65 + b"*\n", 1),
    (b"default drop\ndefault keep\n", 2),                      # two defaults
    (b"default\n", 1),
    (b"default mute\n", 1),
    (b" drop a\n", 1),                                         # a blank in front
    (b"DROP a\n", 1),
    (b"".join(b"drop r%03d\n" % i for i in range(257)), 257),  # too many rules
    (b"".join(b"drop %02d" % i + b"y" * 62 + b"\n" for i in range(64)) + b"keep z\n", 65),   # too many bytes
]


@pytest.mark.parametrize("text,line", BAD_FILES, ids=[str(i) for i in range(len(BAD_FILES))])
def test_parse_text_rejects_with_the_line(pkg, text, line):
    with pytest.raises(pkg.SrError) as e:
        pkg.rules_parse_text(text)
    assert e.value.errno == errno.EINVAL and e.value.line == line
