"""Synthetic routed records for the MTU packing kernels (sr_pack_packets / sr_pack_packets_many), with
no routing in the way: the packing reads (route, length) records, so a test can hand the device and the
oracle any sequence it likes. A plain helper module (no fixtures, no GPU at import):

  builders   one_shard, boundary, boundary2, skewed, round_robin: seeded RECORD_DTYPE arrays whose
             offsets are unique (7 i + 3), so a sort that is unstable or duplicates a line shows;
  next_fit   a second reference, plain Python written from the reference's push_to_downstream
             (sr-main.c:73-83), independent of oracle/sr_oracle.c;
  run_pack   uploads batches between poison, runs the device packing, returns the raw arrays;
  check_pack compares the raw arrays with a reference, whole, and the poison past every end;
  cases_*    the batches tests/test_gpu_pack_records.py runs (tests/test_pack_records.py checks on the
             CPU that both references agree on every one of them).
"""
from __future__ import annotations

import functools

import numpy as np

RECORD_DTYPE = np.dtype([("offset", "<u4"), ("length", "<u2"), ("route", "<u2")])
PACKET_DTYPE = np.dtype([("first", "<u4"), ("nlines", "<u2"), ("shard", "<u2"), ("length", "<u2"),
                         ("carry", "<u2"), ("open", "<u4")])
CAP = 1450                       # DOWNSTREAM_BUF_SIZE (sr-types.h:30)
MINL, MAXL = 6, 1449             # the lengths of a routed line (sr-main.c:180)
UNROUTED = (0xFFFD, 0xFFFE, 0xFFFF)
UNROUTED_LENGTHS = (0, 1, 5, 6, 700, 1449, 1450, 4096, 65535)
PATTERNS = ("six", "max", "pair", "alt", "saw", "rand")
SAW_STRIDE = 389                 # coprime to 1444 = 2^2 19^2: the cycle visits every length 6..1449
POISON = 0xA5
EXTRA = 4                        # entries allocated (and poisoned) past every capacity passed


def _records(routes, lengths):
    r = np.zeros(len(routes), dtype=RECORD_DTYPE)
    r["offset"] = 7 * np.arange(len(routes), dtype=np.uint64) + 3
    r["length"] = lengths
    r["route"] = routes
    r.flags.writeable = False
    return r


def _rand_lengths(rng, count):
    return rng.integers(MINL, MAXL + 1, count)


# ---- builders -----------------------------------------------------------------------------------
def pattern_lengths(count, pattern):
    i = np.arange(count, dtype=np.int64)
    if pattern == "six":         # 241 lines a packet
        return np.full(count, 6, dtype=np.int64)
    if pattern == "max":         # one line a packet, one line length: no next() search
        return np.full(count, MAXL, dtype=np.int64)
    if pattern == "pair":        # two lines exactly 1450
        return np.full(count, 725, dtype=np.int64)
    if pattern == "alt":         # one line a packet with lmin = 6: the widest search, a packet per line
        return np.where(i % 2 == 0, MAXL, 6)
    if pattern == "saw":
        return MINL + (i * SAW_STRIDE) % (MAXL - MINL + 1)
    if pattern == "rand":
        return _rand_lengths(np.random.default_rng(0x5A00 + count), count)
    raise ValueError(pattern)


def one_shard(count, pattern, shard=1):
    """`count` lines of one shard with the lengths of `pattern`."""
    return _records(np.full(count, shard, dtype=np.int64), pattern_lengths(count, pattern))


def boundary_lengths(ch, k, L1, seed, at=1):
    rng = np.random.default_rng(seed)
    return np.concatenate([np.full(at * ch - k, MAXL, dtype=np.int64), np.full(k, 6, dtype=np.int64),
                           np.array([L1], dtype=np.int64), _rand_lengths(rng, 300)])


def boundary(ch, k, L1, seed, shard=1, at=1):
    """One shard: at * ch - k lines of 1449 (a packet each), k lines of 6 (one packet, open at line
    at * ch), the line L1 at index at * ch, then 300 seeded random lines. The fill arriving at line
    at * ch is 6 k (1449 for k = 0)."""
    lens = boundary_lengths(ch, k, L1, seed, at)
    return _records(np.full(len(lens), shard, dtype=np.int64), lens)


def boundary2(ch, k, L1, seed, shard=1):
    """boundary() at line 2 ch: the shard's third chunk."""
    return boundary(ch, k, L1, seed, shard, at=2)


def boundary_fill(k):
    return 6 * k if k else MAXL


def boundary_L1(k):
    """{6, exact fit, over by one, 1449} within the routed lengths."""
    x = boundary_fill(k)
    return sorted({v for v in (6, CAP - x, CAP + 1 - x, MAXL) if MINL <= v <= MAXL})


def skewed(n, hot, hot_lines, per_other, p_unrouted, seed, every=1):
    """Shard `hot` gets hot_lines lines, every other shard s with s % every == 0 gets per_other; a
    fraction p_unrouted of all records is unrouted (0xFFFD / 0xFFFE / 0xFFFF, any length). The order is
    a seeded permutation."""
    rng = np.random.default_rng(seed)
    others = np.array([s for s in range(n) if s != hot and s % every == 0], dtype=np.int64)
    routes = np.concatenate([np.full(hot_lines, hot, dtype=np.int64), np.repeat(others, per_other)])
    lengths = _rand_lengths(rng, len(routes))
    nun = int(round(p_unrouted * len(routes) / (1.0 - p_unrouted))) if p_unrouted else 0
    if nun:
        routes = np.concatenate([routes, np.array(UNROUTED, dtype=np.int64)[np.arange(nun) % 3]])
        ul = np.array(UNROUTED_LENGTHS, dtype=np.int64)[np.arange(nun) % len(UNROUTED_LENGTHS)]
        ul = np.where(np.arange(nun) % 2 == 0, ul, rng.integers(0, 65536, nun))
        lengths = np.concatenate([lengths, ul])
    perm = rng.permutation(len(routes))
    return _records(routes[perm], lengths[perm])


def round_robin(n, rounds, seed=0x0B1):
    """route = i % n: every 64-record row of a sort tile holds 64 distinct keys (n >= 64)."""
    rng = np.random.default_rng(seed + n)
    return _records(np.arange(n * rounds, dtype=np.int64) % n, _rand_lengths(rng, n * rounds))


def mixed(n, size, seed):
    """About `size` records over n shards, six tenths of them on one shard, 5 % unrouted."""
    hot_lines = max(1, size * 6 // 10)
    return skewed(n, seed % n, hot_lines, (size - hot_lines) // max(n - 1, 1), 0.05 if size >= 20 else 0.0, seed)


# ---- a batch of a packing launch ----------------------------------------------------------------
class Batch:
    """One sr_pack_batch: the records and what the call is told about them."""

    def __init__(self, recs, n, fill=None, probed=None, max_records=None, n_records=None, max_packets=None,
                 null_recs=False, null_packets=False, alias_fill=False, name=""):
        self.recs = recs
        self.n = n
        self.fill = None if fill is None else np.asarray(fill, dtype=np.uint16)
        assert self.fill is None or (len(self.fill) == n and int(self.fill.max(initial=0)) <= CAP)
        self.probed = None if probed is None else sorted(int(k) for k in probed)   # None: a null bitmap
        self.max_records = len(recs) if max_records is None else max_records
        self.n_records = len(recs) if n_records is None else n_records             # *d_n_records
        assert self.max_records <= len(recs)          # the device may read that many
        self.lines = min(self.n_records, self.max_records)
        self.max_packets = 2 * self.lines + 5 * n + 4 if max_packets is None else max_packets
        self.null_recs, self.null_packets, self.alias_fill = null_recs, null_packets, alias_fill
        assert not null_recs or self.max_records == 0
        assert not null_packets or self.max_packets == 0
        assert not alias_fill or self.fill is not None
        self.name = name
        self._want = None

    def seen(self):
        """The records the call packs: the first min(*d_n_records, max_records)."""
        return self.recs[: self.lines]

    def want(self, ref):
        """ref = oracle.pack_packets (cached) or next_fit."""
        return ref(self.seen(), self.n, self.fill, self.probed or ())


def reference(oracle, b):
    if b._want is None:
        b._want = b.want(oracle.pack_packets)
    return b._want


# ---- the second reference -----------------------------------------------------------------------
def next_fit(recs, n, fill_in=None, probed=()):
    """The reference's packing, line by line. Every valid line is pushed to its downstream in arrival
    order (sr-main.c:103); push_to_downstream (sr-main.c:73-83):
        :75     a line that does not fit behind the pending bytes within 1450 closes the packet
        :77     (the flush; :65 the fill starts again at 0);
        :80-82  the line is appended and the fill grows by its length;
    and a downstream probed while dead loses its buffer (sr-main.c:106). Returns what
    oracle.pack_packets returns: (sorted records, packets, fill_out u16 [n], valid lines)."""
    route = recs["route"].tolist()
    length = recs["length"].tolist()
    groups = [[] for _ in range(n + 1)]
    for i, r in enumerate(route):
        groups[r if r < n else n].append(i)       # arrival order within a key
    dead = set(int(k) for k in probed)
    order, packets, fout = [], [], []
    pos = 0
    for s in range(n):
        fill = int(fill_in[s]) if fill_in is not None else 0
        idx = groups[s]
        if idx:
            pstart, carry, plen = pos, fill, 0
            q = pos
            for i in idx:
                L = length[i]
                if fill + L > CAP:                                  # :75
                    packets.append((pstart, q - pstart, s, plen, carry, 0))   # :77, flushed
                    fill = 0                                        # :65
                    pstart, carry, plen = q, 0, 0
                fill += L                                           # :82
                plen += L
                q += 1
            packets.append((pstart, q - pstart, s, plen, carry, 1))  # the buffer left pending
            pos = q
            order.extend(idx)
        fout.append(0 if s in dead else fill)                       # :106
    n_valid = pos
    order.extend(groups[n])
    srt = recs[np.array(order, dtype=np.int64)] if order else np.zeros(0, dtype=RECORD_DTYPE)
    pk = np.array(packets, dtype=PACKET_DTYPE) if packets else np.zeros(0, dtype=PACKET_DTYPE)
    return srt, pk, np.array(fout, dtype=np.uint16), n_valid


# ---- the device runner --------------------------------------------------------------------------
def _bitmap(n, probed):
    w = np.zeros(max((n + 63) // 64, 1), dtype=np.uint64)
    for k in probed:
        w[k >> 6] |= np.uint64(1) << np.uint64(k & 63)
    return w


def run_pack(pkg, torch, router, batches, single=False, extra=EXTRA, poison=POISON):
    """Pack `batches` (Batch) in one sr_pack_packets_many call (sr_pack_packets with single=True and
    one batch). Everything lives in one device arena filled with the poison byte; d_sorted, d_packets,
    d_counts and d_fill_out are `extra` entries longer than the capacities passed. Returns one dict of
    raw arrays per batch (check_pack's `got`). The inputs must come back unchanged."""
    assert batches and (not single or len(batches) == 1)
    lay, total = [], 0

    def take(nbytes):
        nonlocal total
        at = total
        total += (nbytes + 15) & ~15
        return at

    for b in batches:
        o = {"recs": None if b.null_recs else take(8 * max(len(b.recs), 1)), "n_records": take(8),
             "fill": None if b.fill is None else take(2 * (b.n + extra)),
             "probed": None if b.probed is None else take(8 * max((b.n + 63) // 64, 1)),
             "sorted": None if b.null_recs else take(8 * (b.max_records + extra)),
             "packets": None if b.null_packets else take(16 * (b.max_packets + extra)),
             "counts": take(8 * (3 + extra))}
        o["fill_out"] = o["fill"] if b.alias_fill else take(2 * (b.n + extra))
        lay.append(o)
    host = np.full(total, poison, dtype=np.uint8)

    def put(at, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        host[at: at + raw.size] = raw

    for b, o in zip(batches, lay):
        if o["recs"] is not None:
            put(o["recs"], b.recs)
        put(o["n_records"], np.array([b.n_records], dtype=np.uint64))
        if o["fill"] is not None:
            put(o["fill"], b.fill)
        if o["probed"] is not None:
            put(o["probed"], _bitmap(b.n, b.probed))
    dev = torch.from_numpy(host.copy()).cuda()    # a pageable copy: done when .cuda() returns
    base = dev.data_ptr()
    assert base % 16 == 0

    def ptr(at):
        return 0 if at is None else base + at

    args = [(ptr(o["recs"]), ptr(o["n_records"]), b.max_records, ptr(o["fill"]), ptr(o["probed"]), ptr(o["sorted"]),
             ptr(o["packets"]), b.max_packets, ptr(o["counts"]), ptr(o["fill_out"])) for b, o in zip(batches, lay)]
    if single:
        router.pack_packets(*args[0])
    else:
        router.pack_packets_many(args)
    router.sync()
    torch.cuda.synchronize()
    out = dev.cpu().numpy()
    got = []
    for b, o in zip(batches, lay):
        def view(key, dtype, count):
            if o[key] is None:
                return np.zeros(0, dtype=dtype)
            return out[o[key]: o[key] + count * np.dtype(dtype).itemsize].view(dtype).copy()

        for key, size in (("recs", 8 * len(b.recs)), ("n_records", 8), ("probed", 8 * max((b.n + 63) // 64, 1)),
                          ("fill", 0 if b.alias_fill else 2 * (b.n + extra))):
            if o[key] is not None:
                assert np.array_equal(out[o[key]: o[key] + size], host[o[key]: o[key] + size]), \
                    f"batch {b.name!r}: the call changed its input {key}"
        got.append({"sorted": view("sorted", RECORD_DTYPE, b.max_records + extra),
                    "packets": view("packets", PACKET_DTYPE, b.max_packets + extra),
                    "counts": view("counts", np.uint64, 3 + extra),
                    "fill_out": view("fill_out", np.uint16, b.n + extra),
                    "poison": poison})
    return got


def expected_raw(want, max_records, max_packets, extra=EXTRA, poison=POISON, null_recs=False, null_packets=False):
    """The raw arrays a correct run leaves (run_pack's dict), built from a reference's result."""
    srt, pk, fout, nv = want

    def arena(dtype, count, head):
        a = np.full(count * np.dtype(dtype).itemsize, poison, dtype=np.uint8).view(dtype).copy()
        a[: len(head)] = head
        return a

    npk = min(len(pk), max_packets)
    return {"sorted": np.zeros(0, RECORD_DTYPE) if null_recs else arena(RECORD_DTYPE, max_records + extra, srt),
            "packets": np.zeros(0, PACKET_DTYPE) if null_packets else arena(PACKET_DTYPE, max_packets + extra, pk[:npk]),
            "counts": arena(np.uint64, 3 + extra, np.array([len(pk), nv, len(srt)], dtype=np.uint64)),
            "fill_out": arena(np.uint16, len(fout) + extra, fout),
            "poison": poison}


def _same(what, got, want):
    g = np.ascontiguousarray(got).view(np.uint8).reshape(len(got), got.dtype.itemsize)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(len(want), want.dtype.itemsize)
    assert g.shape == w.shape, f"{what}: {g.shape[0]} entries against {w.shape[0]}"
    if not np.array_equal(g, w):
        k = int(np.flatnonzero((g != w).any(axis=1))[0])
        raise AssertionError(f"{what} differ first at {k}: got {got[k]!r}, want {want[k]!r}")


def _poison(what, arr, poison):
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    bad = np.flatnonzero(raw != poison)
    assert bad.size == 0, f"{what}: byte {int(bad[0]) if bad.size else 0} past the end was written"


def check_pack(got, want, max_records, max_packets):
    """got: run_pack's raw arrays of one batch; want: a reference's (sorted, packets, fill_out, valid
    lines) over the records the call packs. Whole-array compares, and the poison past every end."""
    srt, pk, fout, nv = want
    lines, n, poison = len(srt), len(fout), got["poison"]
    assert lines <= max_records
    counts = got["counts"]
    assert [int(c) for c in counts[:3]] == [len(pk), int(nv), lines], \
        f"counts {[int(c) for c in counts[:3]]}, want {[len(pk), int(nv), lines]}"
    _poison("counts", counts[3:], poison)
    if len(got["sorted"]) == 0:
        assert lines == 0
    else:
        _same("sorted records", got["sorted"][:lines], srt)
        _poison("sorted records", got["sorted"][lines:], poison)
    npk = min(len(pk), max_packets)
    if len(got["packets"]) == 0:
        assert npk == 0
    else:
        _same("packet descriptors", got["packets"][:npk], pk[:npk])
        _poison("packet descriptors", got["packets"][npk:], poison)
    _same("pending bytes after the batch", got["fill_out"][:n], fout)
    _poison("pending bytes after the batch", got["fill_out"][n:], poison)


# ---- the cases of tests/test_gpu_pack_records.py --------------------------------------------------
COUNTS = (1, 241, 242, 2047, 2048, 2049, 4096, 4097, 4607, 4608, 4609, 9216, 9217)
COUNT_FILLS = (0, 1, 725, 1444, 1449, 1450)
CHUNKS = (2048, 4608)
BOUNDARY_K = (0, 1, 120, 240, 241)
BOUNDARY_FILLS = (0, 7, 1450)
SHARD_COUNTS = (64, 65, 1024, 1025, 4096)
UNEVEN_BATCHES = (8, 9, 31, 32)
UNEVEN_SIZES = (1, 63, 64, 65, 300, 1023, 1024, 1025, 2048, 2049, 4609, 7000, 12000)


@functools.lru_cache(maxsize=None)
def cases_counts():
    """(a) every (count, pattern) twice, n = 2, the lines on shard 1; the fill of shard 1 in rotation
    (the two rounds a step apart, so each (count, pattern) meets two fills), shard 0 empty with a fill of
    its own that must pass through. Counts vary fastest: the 32 batches of a launch differ in size."""
    shapes = [(c, p) for p in PATTERNS for c in COUNTS]
    out = []
    for i in range(2 * len(shapes)):
        c, p = shapes[i % len(shapes)]
        f = COUNT_FILLS[(i + i // len(shapes)) % len(COUNT_FILLS)]
        out.append(Batch(one_shard(c, p), 2, fill=[(37 * i + 11) % (CAP + 1), f], name=f"{p}-{c}-fill{f}"))
    return out


@functools.lru_cache(maxsize=None)
def cases_boundary(ch):
    """(b) a packet's exact fit, its overflow by one, a full buffer and a packet of sixes arriving at
    line ch and at line 2 ch of a shard."""
    out = []
    for k in BOUNDARY_K:
        for L1 in boundary_L1(k):
            for at in (1, 2):
                recs = boundary(ch, k, L1, seed=1000 * k + L1, at=at)
                for f in BOUNDARY_FILLS:
                    out.append(Batch(recs, 2, fill=[(k + f) % (CAP + 1), f], name=f"ch{ch}-at{at}-k{k}-L{L1}-fill{f}"))
    return out


def hot_shards(n):
    """Shard 0, shard n - 1, and the slice edges of the 1024-thread kernels where n allows."""
    return sorted({0, n - 1} | {s for s in (1023, 1024) if s < n})


@functools.lru_cache(maxsize=None)
def cases_shards(n, ch):
    """(c) per hot shard a dense batch (hot shard 2.5 chunks, three lines on every other shard, 5 %
    unrouted) and a mostly empty one (three lines on the hot shard and on every 7th); round_robin(n, 3).
    Random fills; two batches in four have a probed-dead bitmap with bits on shards with and without lines."""
    rng = np.random.default_rng(0xC000 + 7 * n + ch)
    out = []

    def add(recs, name, with_lines, without_lines):
        fill = rng.integers(0, CAP + 1, n)
        probed = None
        if len(out) % 4 in (0, 1):
            probed = set(rng.choice(n, max(n // 16, 2), replace=False).tolist())
            probed |= set(with_lines) | set(without_lines)
        out.append(Batch(recs, n, fill=fill, probed=probed, name=f"n{n}-ch{ch}-{name}"))

    for j, hot in enumerate(hot_shards(n)):
        add(skewed(n, hot, int(2.5 * ch), 3, 0.05, seed=n + 31 * j), f"dense-hot{hot}", [hot, (hot + 1) % n], [])
        empty = [s for s in range(n - 1, 0, -1) if s % 7 and s != hot][:2]
        add(skewed(n, hot, 3, 3, 0.05, seed=n + 31 * j + 1, every=7), f"sparse-hot{hot}", [hot, 7], empty)
    add(round_robin(n, 3), "round-robin", [0, n - 1], [])
    return out


@functools.lru_cache(maxsize=None)
def cases_uneven(nb):
    """(d) nb batches of n = 16 with their own fills, from 0 records (max_records = 0, null record
    pointers) to ~12 k; an empty batch first, at index 7, at index 8 and last."""
    n = 16
    rng = np.random.default_rng(0xD000 + nb)
    out = []
    for j in range(nb):
        fill = rng.integers(0, CAP + 1, n)
        probed = None if j % 3 == 0 else rng.choice(n, 3, replace=False).tolist()
        if j in (0, 7, 8, nb - 1):
            # (*d_n_records is not 0 in two of them: max_records = 0 still packs nothing)
            out.append(Batch(np.zeros(0, dtype=RECORD_DTYPE), n, fill=fill, probed=probed, null_recs=True,
                             n_records=1000 if j in (7, nb - 1) else 0, name=f"nb{nb}-{j}-empty"))
        else:
            size = UNEVEN_SIZES[(5 * j + nb) % len(UNEVEN_SIZES)]
            out.append(Batch(mixed(n, size, seed=97 * nb + j), n, fill=fill, probed=probed, name=f"nb{nb}-{j}-size{size}"))
    return out


@functools.lru_cache(maxsize=None)
def cases_capacity():
    """(e) by name; the descriptor capacities come from the packet count of the reference
    (capacity_packets)."""
    n = 8
    rng = np.random.default_rng(0xE000)
    over = mixed(n, 5000, seed=5)
    return {
        "over": Batch(over, n, fill=rng.integers(0, CAP + 1, n), probed=[1, 6], max_records=len(over) - 1000, name="over"),
        "shape": Batch(mixed(n, 3000, seed=6), n, fill=rng.integers(0, CAP + 1, n), probed=[2], name="shape"),
        "none": Batch(mixed(n, 100, seed=7), n, fill=rng.integers(1, CAP + 1, n), probed=[0, 3, 7], n_records=0, name="none"),
        "alias": Batch(skewed(64, 5, 5000, 3, 0.05, seed=8), 64, fill=rng.integers(0, CAP + 1, 64), alias_fill=True,
                       name="alias"),
    }


def capacity_packets(npk):
    """The batches of the max_packets case: {0 with a null d_packets, 1, npk - 1, npk}."""
    shape = cases_capacity()["shape"]
    return [Batch(shape.recs, shape.n, fill=shape.fill, probed=shape.probed, max_packets=m, null_packets=m == 0,
                  name=f"max_packets{m}") for m in (0, 1, npk - 1, npk)]


def per_call(n):
    """Batches per launch: 32, fewer where n + 1 chunks of scratch per batch add up."""
    return max(1, min(32, 20000 // (n + 1)))
