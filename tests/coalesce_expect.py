"""The plain-counter coalescing of include/sr_route.h restated in Python: the grammar of a plain counter, the
direct-mapped groups, the records that come out and the merged text behind the batch. Exact and deterministic:
the kernels and the C functions must agree with this bit for bit."""
from __future__ import annotations

import re

import numpy as np

from stats_expect import RECORD_DTYPE, fmix64, fmix64_inverse, name_hash, records_of  # noqa: F401 (re-exported)

NAME_MAX = 1425
MIN_SLOTS, MAX_SLOTS, DEFAULT_SLOTS = 16, 1 << 22, 65536
MAX_BYTES = 1 << 30
MIN_LINE, MAX_LINE = 6, 1449

# <name>:-?[0-9]{1,9}|c\n with the ':' the line's first one; a name byte is anything but ':'
_PLAIN = re.compile(rb"([^:]{1,%d}):(-?[0-9]{1,9})\|c\n" % NAME_MAX, re.S)


def parse(line: bytes):
    """(name_len, value) when `line` ('\\n' included) is a plain counter, else None."""
    if not MIN_LINE <= len(line) <= MAX_LINE:
        return None
    m = _PLAIN.fullmatch(line)
    return (len(m.group(1)), int(m.group(2))) if m else None


def dec(total: int) -> bytes:
    return b"%d" % total


def merged_line(name: bytes, total: int) -> bytes:
    return name + b":" + dec(total) + b"|c\n"


def append_capacity(nbytes: int) -> int:
    return nbytes


class Result:
    """What sr_coalesce leaves for one batch: the records out, the four counts, the whole merged text and the
    part of it that is written (its first min(len, append_cap) bytes)."""

    def __init__(self, out, counts, text, append_cap):
        self.out, self.counts, self.text = out, counts, text
        self.written = text[:append_cap]
        self.complete = len(text) <= append_cap


def coalesce(data: bytes, recs, hashes, n_downstreams: int, slots: int = DEFAULT_SLOTS, append_cap: int | None = None,
             n_records: int | None = None, max_records: int | None = None) -> Result:
    nbytes = len(data)
    append_cap = append_capacity(nbytes) if append_cap is None else append_cap
    max_records = len(recs) if max_records is None else max_records
    n = min(len(recs) if n_records is None else n_records, max_records)
    assert n <= len(recs) and slots & (slots - 1) == 0
    recs = np.asarray(recs, RECORD_DTYPE)[:n]
    hashes = [int(h) for h in np.asarray(hashes, np.uint64)[:n]]
    plain = [None] * n                     # (k, v, name) of the plain counters
    owner = {}                             # slot -> the lowest plain index
    slot_of = [0] * n
    for i in range(n):
        o, ln, r = int(recs[i]["offset"]), int(recs[i]["length"]), int(recs[i]["route"])
        if r >= n_downstreams or o + ln > nbytes:
            continue
        p = parse(data[o:o + ln])
        if p is None:
            continue
        plain[i] = (p[0], p[1], data[o:o + p[0]])
        slot_of[i] = fmix64(hashes[i]) & (slots - 1)
        owner.setdefault(slot_of[i], i)
    members = {}                           # owner index -> the indices that joined it, itself first
    for i in range(n):
        if plain[i] is None:
            continue
        o = owner[slot_of[i]]
        if hashes[i] == hashes[o] and int(recs[i]["route"]) == int(recs[o]["route"]) and plain[i][0] == plain[o][0] \
                and plain[i][2] == plain[o][2]:
            members.setdefault(o, []).append(i)
    dropped = {i for o, g in members.items() if len(g) >= 2 for i in g if i != o}
    out = np.zeros(n - len(dropped), RECORD_DTYPE)
    text = bytearray()
    groups = 0
    at = 0
    for i in range(n):
        if i in dropped:
            continue
        out[at] = recs[i]
        g = members.get(i)
        if g is not None and len(g) >= 2:
            line = merged_line(plain[i][2], sum(plain[x][1] for x in g))
            out[at]["offset"] = (nbytes + len(text)) & 0xFFFFFFFF
            out[at]["length"] = len(line)
            text += line
            groups += 1
        at += 1
    counts = np.array([len(out), len(dropped), groups, len(text)], np.uint64)
    return Result(out, counts, bytes(text), append_cap)


def line_of(data: bytes, res: Result, rec) -> bytes:
    """The bytes a record of `res.out` points at: the batch, or the merged text behind it."""
    whole = data + res.text
    o, ln = int(rec["offset"]), int(rec["length"])
    return whole[o:o + ln]


def ledger(lines_with_routes):
    """({(route, name): sum} over the plain counters, [(route, line), ...] of every other line in order)."""
    sums, rest = {}, []
    for route, line in lines_with_routes:
        p = parse(line)
        if p is None:
            rest.append((route, line))
        else:
            key = (route, line[:p[0]])
            sums[key] = sums.get(key, 0) + p[1]
    return sums, rest
