"""The name rules of include/sr_route.h restated in Python: validation of a rule set, the brute-force longest match
over all rules, the compaction of a batch's records and the hits. Exact and deterministic: the kernels and the C
functions must agree with this bit for bit. Nothing here is clever on purpose: every rule is tried on every line."""
from __future__ import annotations

import numpy as np

from stats_expect import RECORD_DTYPE, name_hash, records_of  # noqa: F401 (re-exported)

RULES_MAX, PATTERN_MAX, TEXT_MAX = 256, 64, 4096
NOT_SUBJECT = 0xFFFF
PREFIX, EXACT = 0, 1
DROP, KEEP = 0, 1


def check(rules, default_action=KEEP) -> bool:
    """True when the set is valid. `rules` is [(pattern bytes, kind, action), ...]."""
    if len(rules) > RULES_MAX or default_action not in (DROP, KEEP):
        return False
    seen = set()
    for p, kind, action in rules:
        if not 1 <= len(p) <= PATTERN_MAX or b":" in p or b"\n" in p:
            return False
        if kind not in (PREFIX, EXACT) or action not in (DROP, KEEP) or (kind, p) in seen:
            return False
        seen.add((kind, p))
    return sum(len(p) for p, _, _ in rules) <= TEXT_MAX


def matches(rule, line: bytes) -> bool:
    """The header's definition, on the bytes of one line of L = len(line) bytes."""
    p, kind, _ = rule
    L = len(line)
    if kind == PREFIX:
        return len(p) <= L - 1 and line[:len(p)] == p
    return len(p) + 1 <= L - 1 and line[:len(p)] == p and line[len(p)] == ord(":")


def match(rules, line: bytes) -> int:
    """The winning rule's index: the longest matching pattern, EXACT before PREFIX of one text; len(rules) for
    none."""
    best, key = len(rules), None
    for i, r in enumerate(rules):
        if matches(r, line):
            k = (len(r[0]), r[1])          # EXACT = 1 > PREFIX = 0
            if key is None or k > key:
                best, key = i, k
    return best


class Result:
    """What sr_rules leaves for one batch."""

    def __init__(self, out, hashes_out, match_idx, counts, hits):
        self.out, self.hashes_out, self.match, self.counts, self.hits = out, hashes_out, match_idx, counts, hits


def apply(data: bytes, recs, hashes, n_downstreams: int, rules, default_action=KEEP, n_records=None,
          max_records=None) -> Result:
    """The stage over one batch. `hashes` may be None. hits is an (len(rules) + 1, 2) array of {lines, bytes}."""
    nbytes = len(data)
    max_records = len(recs) if max_records is None else max_records
    n = min(len(recs) if n_records is None else n_records, max_records)
    assert n <= len(recs)
    recs = np.asarray(recs, RECORD_DTYPE)[:n]
    actions = [a for _, _, a in rules] + [default_action]
    idx = np.full(n, NOT_SUBJECT, np.uint16)
    hits = np.zeros((len(rules) + 1, 2), np.uint64)
    keep = np.ones(n, bool)
    dropped_bytes = subject = 0
    for i in range(n):
        o, ln, r = int(recs[i]["offset"]), int(recs[i]["length"]), int(recs[i]["route"])
        if not (r < n_downstreams and ln >= 1 and o + ln <= nbytes):
            continue
        m = match(rules, data[o:o + ln])
        idx[i] = m
        subject += 1
        hits[m, 0] += 1
        hits[m, 1] += ln
        if actions[m] == DROP:
            keep[i] = False
            dropped_bytes += ln
    out = recs[keep].copy()
    hashes_out = None if hashes is None else np.asarray(hashes, np.uint64)[:n][keep].copy()
    counts = np.array([len(out), n - len(out), dropped_bytes, subject], np.uint64)
    return Result(out, hashes_out, idx, counts, hits)
