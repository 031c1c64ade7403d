"""The line grammar of include/sr_route.h restated in Python, from the contract's text with bytes.split and re: the
judgement of one line, the configuration's check, the compaction of a batch's records and the hits per reason.
Exact and deterministic: the kernels and the C functions must agree with this bit for bit. It is no port of the C
function (which walks 16-byte steps with masks), so the two check each other."""
from __future__ import annotations

import re

import numpy as np

from stats_expect import RECORD_DTYPE, name_hash, records_of  # noqa: F401 (re-exported)

(OK, NO_COLON, EMPTY_NAME, NAME_BYTE, NO_TYPE, TYPE, VALUE, SECTION, RATE, TAGS, REASONS) = range(11)
NOT_SUBJECT = 0xFF
NAMES = ["ok", "no_colon", "empty_name", "name_byte", "no_type", "type", "value", "section", "rate", "tags"]
TYPE_BITS = {b"c": 1, b"g": 2, b"ms": 4, b"h": 8, b"s": 16, b"d": 32}
TYPES_ALL = 63
DROP_ALL = 0x3FE

TB = rb"[\x21-\x7b\x7d\x7e]"                 # 0x21..0x7E except '|'
NB_ONLY = re.compile(rb"[\x21-\x39\x3b-\x7b\x7d\x7e]*", re.S)   # TB except ':'
NUMBER = rb"[0-9]{1,20}(?:\.[0-9]{1,20})?"
VALUE_RE = {
    b"c": re.compile(rb"-?" + NUMBER, re.S),
    b"g": re.compile(rb"[+-]?" + NUMBER, re.S),
    b"ms": re.compile(NUMBER, re.S),
    b"h": re.compile(NUMBER, re.S),
    b"d": re.compile(NUMBER, re.S),
    b"s": re.compile(TB + rb"{1,64}", re.S),
}
RATE_RE = re.compile(NUMBER, re.S)
TAGS_RE = re.compile(TB + rb"+", re.S)


def check(drop_mask: int, accept_types: int) -> bool:
    """True when the configuration is valid."""
    if drop_mask & 1 or drop_mask >> REASONS or drop_mask < 0:
        return False
    return accept_types != 0 and not accept_types & ~TYPES_ALL


def judge(line: bytes, accept_types: int = TYPES_ALL) -> int:
    """The reason of one line of L = len(line) >= 1 bytes."""
    c = line[:-1] if line.endswith(b"\n") else line
    p = c.find(b":")
    if p < 0:
        return NO_COLON
    if p == 0:
        return EMPTY_NAME
    if not NB_ONLY.fullmatch(c[:p]):
        return NAME_BYTE
    f = c[p + 1:].split(b"|")
    if len(f) == 1:
        return NO_TYPE
    if not TYPE_BITS.get(f[1], 0) & accept_types:
        return TYPE
    if not VALUE_RE[f[1]].fullmatch(f[0]):
        return VALUE
    seen = b""
    for x in f[2:]:
        lead = x[:1]
        if lead not in (b"@", b"#") or lead in seen or (lead == b"@" and b"#" in seen):
            return SECTION
        seen += lead
        if lead == b"@":
            if not RATE_RE.fullmatch(x[1:]) or f[1] not in (b"c", b"ms", b"h", b"d"):
                return RATE
        elif not TAGS_RE.fullmatch(x[1:]):
            return TAGS
    return OK


def parse_spec(text: str):
    """(drop_mask, accept_types) of an SR_VALIDATE spec, None for a bad one."""
    if text == "count":
        return 0, TYPES_ALL
    if text == "drop":
        return DROP_ALL, TYPES_ALL
    mask = 0
    for name in text.split(","):
        if name not in NAMES[1:]:
            return None
        mask |= 1 << NAMES.index(name)
    return mask, TYPES_ALL


class Result:
    """What sr_validate leaves for one batch."""

    def __init__(self, out, hashes_out, reason, counts, hits):
        self.out, self.hashes_out, self.reason, self.counts, self.hits = out, hashes_out, reason, counts, hits


def apply(data: bytes, recs, hashes, n_downstreams: int, drop_mask=0, accept_types=TYPES_ALL, n_records=None,
          max_records=None) -> Result:
    """The stage over one batch. `hashes` may be None. hits is a (REASONS, 2) array of {lines, bytes}."""
    nbytes = len(data)
    max_records = len(recs) if max_records is None else max_records
    n = min(len(recs) if n_records is None else n_records, max_records)
    assert n <= len(recs)
    recs = np.asarray(recs, RECORD_DTYPE)[:n]
    reason = np.full(n, NOT_SUBJECT, np.uint8)
    hits = np.zeros((REASONS, 2), np.uint64)
    keep = np.ones(n, bool)
    dropped_bytes = subject = 0
    for i in range(n):
        o, ln, r = int(recs[i]["offset"]), int(recs[i]["length"]), int(recs[i]["route"])
        if not (r < n_downstreams and ln >= 1 and o + ln <= nbytes):
            continue
        m = judge(data[o:o + ln], accept_types)
        reason[i] = m
        subject += 1
        hits[m, 0] += 1
        hits[m, 1] += ln
        if drop_mask >> m & 1:
            keep[i] = False
            dropped_bytes += ln
    out = recs[keep].copy()
    hashes_out = None if hashes is None else np.asarray(hashes, np.uint64)[:n][keep].copy()
    counts = np.array([len(out), n - len(out), dropped_bytes, subject], np.uint64)
    return Result(out, hashes_out, reason, counts, hits)


# About ten lines that together use every section: the mutation corpus of the ABI and the GPU tests.
SEED_LINES = [
    b"svc.req:1|c\n",
    b"svc.req.count:12.5|ms|@0.25\n",
    b"a.b:-3.25|c|@1|#env:prod,zone:a\n",
    b"gauge.x:+17|g|#t\n",
    b"users.uniq:alice:bob|s\n",
    b"lat:00000000000000000020.00000000000000000020|h|@0.1|#k:v\n",
    b"dist.v:7|d|@0.5\n",
    b"n:0|g",
    b"a-very.long_name/with~bytes:18446744073709551615|c|#a,b,c\n",
    b"x:1|ms|#only\n",
]


def mutations(lines=SEED_LINES):
    """Every truncation of every line (1 byte or more), and a generator over every single-byte mutation."""
    for ln in lines:
        for k in range(1, len(ln) + 1):
            yield ln[:k]
        for at in range(len(ln)):
            for v in range(256):
                if v != ln[at]:
                    yield ln[:at] + bytes([v]) + ln[at + 1:]
