"""The name statistics of include/sr_route.h restated in numpy: what sr_stats_update leaves in a context, what
sr_stats_read returns (ordering included), and the host-only functions on a snapshot (estimate, cardinality,
merge). Exact and deterministic: the kernels and the C functions must agree with this bit for bit."""
from __future__ import annotations

import math

import numpy as np

DEFAULTS = dict(hll_p=10, cms_rows=4, cms_width=4096, hot_slots=256, hot_div=256, hot_min_lines=1024)
NAME_MAX = 108
ALL = 0xFFFFFFFF
HOT_DTYPE = np.dtype([("hash", "<u8"), ("lines", "<u8"), ("name_len", "<u4"), ("name", "u1", (NAME_MAX,))])
RECORD_DTYPE = np.dtype([("offset", "<u4"), ("length", "<u2"), ("route", "<u2")])
M64 = (1 << 64) - 1


def resolve(cfg: dict | None) -> dict:
    c = dict.fromkeys(DEFAULTS, 0)
    c.update(cfg or {})
    return dict(DEFAULTS) if not any(c.values()) else c


def name_hash(name: bytes) -> int:
    """sr-main.c:120-134: sdbm with signed char."""
    h = 0
    for b in name:
        h = ((h << 6) + (h << 16) - h + (b - 256 if b >= 128 else b)) & M64
    return h


def fmix64(m):
    """The MurmurHash3 finaliser on a u64 array (or an int)."""
    scalar = not isinstance(m, np.ndarray)
    m = np.atleast_1d(np.asarray(m, dtype=np.uint64)).copy()
    with np.errstate(over="ignore"):
        m ^= m >> np.uint64(33)
        m *= np.uint64(0xff51afd7ed558ccd)
        m ^= m >> np.uint64(33)
        m *= np.uint64(0xc4ceb9fe1a85ec53)
        m ^= m >> np.uint64(33)
    return int(m[0]) if scalar else m


def fmix64_inverse(m: int) -> int:
    """The hash whose fmix64 is m (for made-up hashes that land where a test wants them)."""
    inv1, inv2 = pow(0xc4ceb9fe1a85ec53, -1, 1 << 64), pow(0xff51afd7ed558ccd, -1, 1 << 64)
    unshift = lambda x: x ^ (x >> 33)   # x ^= x >> 33 is its own inverse on 64 bits (33 * 2 >= 64)
    m = unshift(m)
    m = (m * inv1) & M64
    m = unshift(m)
    m = (m * inv2) & M64
    return unshift(m)


def _clz64(w):
    """Leading zeros of non-zero u64 values."""
    w = w.copy()
    n = np.zeros(w.shape, np.uint64)
    for s in (32, 16, 8, 4, 2, 1):
        top0 = (w >> np.uint64(64 - s)) == 0
        n += np.where(top0, np.uint64(s), np.uint64(0))
        w = np.where(top0, w << np.uint64(s), w)
    return n


def hll_place(m, p: int):
    """(register index, rho) of mixed hashes m."""
    idx = (m >> np.uint64(64 - p)).astype(np.int64)
    w = m << np.uint64(p)
    rho = np.where(w == 0, np.uint64(64 - p + 1), _clz64(np.where(w == 0, np.uint64(1), w)) + np.uint64(1))
    return idx, rho.astype(np.uint8)


def cms_cells(m, rows: int, width: int):
    """[rows, len(m)] cell indices."""
    a = m & np.uint64(0xFFFFFFFF)
    b = (m >> np.uint64(32)) | np.uint64(1)
    return np.stack([((a + np.uint64(r) * b) & np.uint64(width - 1)).astype(np.int64) for r in range(rows)])


def line_name(data: bytes, offset: int, length: int) -> bytes:
    """The bytes before the first ':' inside the line clipped to the batch."""
    start, end = min(offset, len(data)), min(offset + length, len(data))
    seg = data[start:end]
    k = seg.find(b":")
    return seg if k < 0 else seg[:k]


class Snap:
    """A snapshot: the fields of sr_stats_snapshot."""

    def __init__(self, cfg: dict, n: int):
        self.cfg, self.n = dict(cfg), n
        self.lines = np.zeros(4, np.uint64)
        self.bytes = np.zeros(4, np.uint64)
        self.ignored = 0
        self.hot_overflow = 0
        self.shard_lines = np.zeros(n, np.uint64)
        self.shard_bytes = np.zeros(n, np.uint64)
        self.regs = np.zeros((n, 1 << cfg["hll_p"]), np.uint8)
        self.cells = np.zeros((cfg["cms_rows"], cfg["cms_width"]), np.uint64)
        self.hot = np.zeros(0, HOT_DTYPE)

    @property
    def total(self) -> int:
        return int(self.lines[0])


def estimate(snap, h: int) -> int:
    c = cms_cells(np.array([fmix64(h)], np.uint64), snap.cfg["cms_rows"], snap.cfg["cms_width"])[:, 0]
    return int(min(int(snap.cells[r, c[r]]) for r in range(snap.cfg["cms_rows"])))


def cardinality(snap, shard: int = ALL) -> float:
    regs = snap.regs.max(axis=0) if shard == ALL and snap.n else \
        np.zeros(1 << snap.cfg["hll_p"], np.uint8) if shard == ALL else snap.regs[shard]
    m = regs.size
    s = float(np.sum(np.ldexp(1.0, -regs.astype(np.int64))))
    zeros = int((regs == 0).sum())
    alpha = {16: 0.673, 32: 0.697, 64: 0.709}.get(m, 0.7213 / (1.0 + 1.079 / m))
    e = alpha * m * m / s
    if e <= 2.5 * m and zeros:
        return m * math.log(m / zeros)
    return e


def sort_hot(snap) -> None:
    """lines = est(hash) from this snapshot; by lines descending, then hash ascending."""
    hot = snap.hot.copy()
    for e in hot:
        e["lines"] = estimate(snap, int(e["hash"]))
    order = sorted(range(len(hot)), key=lambda i: (-int(hot[i]["lines"]), int(hot[i]["hash"])))
    snap.hot = hot[order]


def hot_entry(h: int, name: bytes) -> np.ndarray:
    e = np.zeros(1, HOT_DTYPE)
    e["hash"], e["name_len"] = h, len(name)
    keep = np.frombuffer(name[:NAME_MAX], np.uint8)
    e["name"][0, : keep.size] = keep
    return e


def merge(into, other) -> None:
    assert into.cfg == other.cfg and into.n == other.n
    into.lines += other.lines
    into.bytes += other.bytes
    into.ignored += other.ignored
    into.shard_lines += other.shard_lines
    into.shard_bytes += other.shard_bytes
    np.maximum(into.regs, other.regs, out=into.regs)
    into.cells += other.cells
    into.hot_overflow = 1 if (into.hot_overflow or other.hot_overflow) else 0
    have = set(int(h) for h in into.hot["hash"])
    add = []
    for e in other.hot:
        if int(e["hash"]) in have:
            continue
        if len(have) >= into.cfg["hot_slots"]:
            into.hot_overflow = 1
            continue
        have.add(int(e["hash"]))
        add.append(e)
    if add:
        into.hot = np.concatenate([into.hot, np.array(add, HOT_DTYPE)])
    sort_hot(into)


class Stats:
    """The state of one context. update() takes the batches of one call: (data, records, hashes[, n_records
    [, max_records]]), n_records being the device's count (it may exceed max_records)."""

    def __init__(self, n: int, cfg: dict | None = None):
        self.cfg, self.n = resolve(cfg), n
        self.reset()

    def reset(self) -> None:
        self.s = Snap(self.cfg, self.n)
        self.names: dict[int, bytes] = {}   # the hot table: hash -> name, in insertion order

    def update(self, batches) -> None:
        s, cfg, n = self.s, self.cfg, self.n
        kept = []
        for b in batches:
            data, recs, hashes = bytes(b[0]), np.asarray(b[1]), np.asarray(b[2], dtype=np.uint64)
            max_records = b[4] if len(b) > 4 and b[4] is not None else len(recs)
            n_records = b[3] if len(b) > 3 and b[3] is not None else len(recs)
            k = min(n_records, max_records)
            r, h = recs[:k], hashes[:k]
            route, length = r["route"].astype(np.int64), r["length"].astype(np.uint64)
            valid = route < n
            for v, code in ((1, 0xFFFD), (2, 0xFFFE), (3, 0xFFFF)):
                s.lines[v] += np.uint64(int((route == code).sum()))
                s.bytes[v] += length[route == code].sum(dtype=np.uint64)
            s.lines[0] += np.uint64(int(valid.sum()))
            s.bytes[0] += length[valid].sum(dtype=np.uint64)
            s.ignored += int((~valid & (route < 0xFFFD)).sum())
            sh, m = route[valid], fmix64(h[valid])
            np.add.at(s.shard_lines, sh, np.uint64(1))
            np.add.at(s.shard_bytes, sh, length[valid])
            idx, rho = hll_place(m, cfg["hll_p"])
            np.maximum.at(s.regs, (sh, idx), rho)
            cells = cms_cells(m, cfg["cms_rows"], cfg["cms_width"])
            for row in range(cfg["cms_rows"]):
                np.add.at(s.cells[row], cells[row], np.uint64(1))
            kept.append((data, r[valid], h[valid], cells))
        # hot names: settled after every record of the call has been counted
        total = s.total
        T = max(cfg["hot_min_lines"], -(-total // cfg["hot_div"]))
        for data, r, h, cells in kept:
            if not len(r):
                continue
            est = np.min(np.stack([s.cells[row][cells[row]] for row in range(cfg["cms_rows"])]), axis=0)
            for i in np.nonzero(est >= np.uint64(T))[0]:
                hh = int(h[i])
                if hh in self.names:
                    continue
                if len(self.names) >= cfg["hot_slots"]:
                    s.hot_overflow = 1
                    continue
                self.names[hh] = line_name(data, int(r["offset"][i]), int(r["length"][i]))

    def threshold(self) -> int:
        return max(self.cfg["hot_min_lines"], -(-self.s.total // self.cfg["hot_div"]))

    def read(self) -> Snap:
        out = Snap(self.cfg, self.n)
        for f in ("lines", "bytes", "shard_lines", "shard_bytes", "regs", "cells"):
            setattr(out, f, getattr(self.s, f).copy())
        out.ignored, out.hot_overflow = self.s.ignored, self.s.hot_overflow
        if self.names:
            out.hot = np.concatenate([hot_entry(h, nm) for h, nm in self.names.items()])
        sort_hot(out)
        return out


def records_of(lines, n: int, route_of=None):
    """A framed batch and its records and hashes from a list of lines (bytes without '\\n'): every line with a
    ':' and 6..1449 bytes is valid and goes to shard route_of(hash) (default hash % n)."""
    data = b"".join(l + b"\n" for l in lines)
    recs = np.zeros(len(lines), RECORD_DTYPE)
    hashes = np.zeros(len(lines), np.uint64)
    off = 0
    for i, l in enumerate(lines):
        ln = len(l) + 1
        recs[i]["offset"], recs[i]["length"] = off, min(ln, 0xFFFF)
        k = l.find(b":")
        if not 5 < ln < 1450:
            recs[i]["route"] = 0xFFFD
        elif k < 0:
            recs[i]["route"] = 0xFFFE
        elif n == 0:
            recs[i]["route"] = 0xFFFF
        else:
            hashes[i] = name_hash(l[:k])
            recs[i]["route"] = route_of(int(hashes[i])) if route_of else int(hashes[i]) % n
        off += ln
    return data, recs, hashes


def same(got, exp, overflow_ok: bool = False) -> list[str]:
    """The fields in which two snapshots differ (empty: identical). With overflow_ok the hot entries of an
    overflowed table are not compared (which names found room is not specified)."""
    bad = []
    if dict(got.cfg) != dict(exp.cfg) or got.n != exp.n:
        bad.append("cfg")
    for f in ("lines", "bytes", "shard_lines", "shard_bytes", "regs", "cells"):
        if not np.array_equal(np.asarray(getattr(got, f)), getattr(exp, f)):
            bad.append(f)
    if int(got.ignored) != int(exp.ignored):
        bad.append("ignored")
    if int(got.hot_overflow) != int(exp.hot_overflow):
        bad.append("hot_overflow")
    if not (overflow_ok and exp.hot_overflow):
        g, e = np.asarray(got.hot), exp.hot
        if len(g) != len(e) or any(not np.array_equal(g[f], e[f]) for f in ("hash", "lines", "name_len", "name")):
            bad.append("hot")
    return bad


def to_pkg(pkg, snap):
    """The snapshot as the package's StatsSnapshot (numpy arrays behind a C sr_stats_snapshot)."""
    s = pkg.StatsSnapshot(snap.cfg, snap.n)
    s.lines[:], s.bytes[:] = snap.lines, snap.bytes
    s.ignored, s.hot_overflow = int(snap.ignored), int(snap.hot_overflow)
    s.shard_lines[:], s.shard_bytes[:] = snap.shard_lines, snap.shard_bytes
    s.regs[:], s.cells[:] = snap.regs, snap.cells
    s.set_hot(snap.hot)
    return s
