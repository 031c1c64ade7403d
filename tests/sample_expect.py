"""The sample-rate stage of include/sr_route.h restated in Python, from the contract's text with bytes methods:
whether a line is sampleable and where the rate goes in, the ladder, the keep rule, the rewrite, the stage over one
batch and the hits per step. Exact and deterministic: the kernels and the C functions must agree with this bit for
bit. It calls no library and is no port of the C functions (which walk 16-byte steps with masks), so the two check
each other."""
from __future__ import annotations

import numpy as np

from stats_expect import RECORD_DTYPE, name_hash, records_of  # noqa: F401 (re-exported)

STEPS = 13
K = [1, 2, 5, 10, 20, 50, 100, 200, 500, 1000, 2000, 5000, 10000]
R = [b"", b"0.5", b"0.2", b"0.1", b"0.05", b"0.02", b"0.01", b"0.005", b"0.002", b"0.001", b"0.0005", b"0.0002",
     b"0.0001"]
EXTRA_MAX = 8
LINE_MAX = 1441
NOT_SAMPLEABLE = 0xFF
DROPPED = 0x80
TYPE_BITS = {b"c": 1, b"ms": 4, b"h": 8, b"d": 32}
TYPES_ALL = 1 | 4 | 8 | 32
TYPES_DEFAULT = 4 | 8 | 32
DEFAULT_SLOTS = 65536
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def append_capacity(nbytes: int) -> int:
    """SR_SAMPLE_APPEND_CAPACITY."""
    return nbytes + (nbytes // 6) * 8


def fmix64(m: int) -> int:
    """The MurmurHash3 finaliser."""
    m &= M64
    m ^= m >> 33
    m = m * 0xFF51AFD7ED558CCD & M64
    m ^= m >> 33
    m = m * 0xC4CEB9FE1A85EC53 & M64
    m ^= m >> 33
    return m


def check(slots: int, limit: int, types: int, reserved: int = 0) -> bool:
    """True when the configuration is valid."""
    s = slots or DEFAULT_SLOTS
    if s < 16 or s > 1 << 22 or s & (s - 1):
        return False
    return limit >= 1 and reserved == 0 and types != 0 and not types & ~TYPES_ALL


def parse(line: bytes, types: int = TYPES_ALL):
    """(ins, type bit) of a sampleable line of L = len(line) bytes, None for any other."""
    if not 6 <= len(line) <= LINE_MAX or not line.endswith(b"\n"):
        return None
    c = line[:-1]
    p = c.find(b":")
    if p < 1:
        return None
    q = c.find(b"|", p + 1)
    if q < 0 or q == p + 1:
        return None
    e = c.find(b"|", q + 1)
    if e < 0:
        e = len(c)
    bit = TYPE_BITS.get(c[q + 1:e], 0) & types
    if not bit:
        return None
    if e != len(c) and not (e + 1 < len(c) and c[e + 1:e + 2] == b"#"):
        return None
    return e, bit


def step(limit: int, c: int) -> int:
    for j in range(STEPS):
        if c <= limit * K[j]:
            return j
    return STEPS - 1


def keep(h: int, seed: int, index: int, j: int) -> bool:
    if j == 0:
        return True
    u = fmix64(h ^ ((seed + index * GOLDEN) & M64))
    return ((u >> 32) * K[j]) >> 32 == 0


def keep_many(h: int, seed: int, indices, j: int):
    """keep() for an array of record indices, in numpy's wrapping u64 arithmetic (for the tests of the kept share)."""
    if j == 0:
        return np.ones(len(indices), bool)
    m = np.asarray(indices).astype(np.uint64)
    with np.errstate(over="ignore"):
        m = np.uint64(h) ^ (np.uint64(seed) + m * np.uint64(GOLDEN))
        m ^= m >> np.uint64(33)
        m *= np.uint64(0xFF51AFD7ED558CCD)
        m ^= m >> np.uint64(33)
        m *= np.uint64(0xC4CEB9FE1A85EC53)
        m ^= m >> np.uint64(33)
        return ((m >> np.uint64(32)) * np.uint64(K[j])) >> np.uint64(32) == 0


def rewrite(line: bytes, ins: int, j: int) -> bytes:
    return line[:ins] + b"|@" + R[j] + line[ins:]


def parse_spec(text: str):
    """(limit, types) of an SR_SAMPLE spec, None for a bad one."""
    head, sep, tail = text.partition(":")
    if not head or not all(ch in "0123456789" for ch in head) or not 1 <= int(head) <= 0xFFFFFFFF:
        return None
    if not sep:
        return int(head), TYPES_DEFAULT
    types = 0
    for name in tail.split(","):
        if name.encode() not in TYPE_BITS:
            return None
        types |= TYPE_BITS[name.encode()]
    return int(head), types


class Result:
    """What sr_sample leaves for one batch."""

    def __init__(self, out, hashes_out, steps, counts, hits, text):
        self.out, self.hashes_out, self.steps, self.counts, self.hits, self.text = out, hashes_out, steps, counts, hits, text

    def written(self, append_cap: int) -> bytes:
        """The bytes of the text that a call with `append_cap` of room writes."""
        return self.text[:append_cap]


def apply(data: bytes, recs, hashes, n_downstreams: int, limit: int, types=TYPES_DEFAULT, slots=0, seed=0,
          n_records=None, max_records=None) -> Result:
    """The stage over one batch; `seed` is cfg.seed + seed_add. hits is a (STEPS, 2) array of {seen, kept}."""
    nbytes = len(data)
    smask = (slots or DEFAULT_SLOTS) - 1
    max_records = len(recs) if max_records is None else max_records
    n = min(len(recs) if n_records is None else n_records, max_records)
    assert n <= len(recs)
    recs = np.asarray(recs, RECORD_DTYPE)[:n]
    hashes = [int(x) for x in np.asarray(hashes, np.uint64)[:n]]
    parsed = [None] * n
    count = {}
    for i in range(n):
        o, ln, r = int(recs[i]["offset"]), int(recs[i]["length"]), int(recs[i]["route"])
        if r < n_downstreams and ln >= 1 and o + ln <= nbytes:
            parsed[i] = parse(data[o:o + ln], types)
            if parsed[i] is not None:
                s = fmix64(hashes[i]) & smask
                count[s] = count.get(s, 0) + 1
    steps = np.full(n, NOT_SAMPLEABLE, np.uint8)
    hits = np.zeros((STEPS, 2), np.uint64)
    out = np.zeros(n, RECORD_DTYPE)
    hashes_out = np.zeros(n, np.uint64)
    text = bytearray()
    m = dropped = rewritten = 0
    for i in range(n):
        rec = recs[i].copy()
        if parsed[i] is not None:
            j = step(limit, count[fmix64(hashes[i]) & smask])
            kept = keep(hashes[i], seed, i, j)
            hits[j, 0] += 1
            hits[j, 1] += kept
            steps[i] = j | (0 if kept else DROPPED)
            if not kept:
                dropped += 1
                continue
            if j:
                o, ln = int(rec["offset"]), int(rec["length"])
                new = rewrite(data[o:o + ln], parsed[i][0], j)
                rec["offset"] = (nbytes + len(text)) & 0xFFFFFFFF
                rec["length"] = len(new)
                text += new
                rewritten += 1
        out[m] = rec
        hashes_out[m] = hashes[i]
        m += 1
    counts = np.array([m, dropped, rewritten, len(text)], np.uint64)
    return Result(out[:m].copy(), hashes_out[:m].copy(), steps, counts, hits, bytes(text))


def lines_of(data: bytes, text: bytes, out) -> list:
    """The lines that the records `out` name, in the batch or, from offset len(data) on, in the rewritten text."""
    whole = data + text
    return [whole[int(r["offset"]):int(r["offset"]) + int(r["length"])] for r in out]


# Lines that together use every type and section: the mutation corpus of the ABI and the GPU tests.
SEED_LINES = [
    b"svc.req:1|c\n",
    b"svc.req.time:12.5|ms\n",
    b"a.b:3.25|h|#env:prod,zone:a\n",
    b"dist.v:7|d|@0.5\n",
    b"lat.p:0020.0020|ms|#k:v,a:b|x\n",
    b"gauge.x:+17|g|#t\n",
    b"a-long.name_with/bytes~in.it:18446744073709551615|ms|#a,b,c\n",
    b"x:1|ms||#t\n",
]
