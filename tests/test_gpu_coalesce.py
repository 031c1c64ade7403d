"""GPU: sr_coalesce, plain counters coalesced on the device, against tests/coalesce_expect.py. Records and hashes
come from the restatement's own tokeniser (names hashed as the oracle hashes them) or are made up, so the stage is
driven alone. Every buffer lies between guard bytes and is compared whole: the records out and the room behind
them, the four counts, the batch, the merged text behind it and the room up to append_cap and past it, and the
inputs, which must come back unchanged."""
from __future__ import annotations

import ctypes
import errno

import numpy as np
import pytest

import coalesce_expect as E

pytestmark = pytest.mark.gpu

GUARD, POISON = 64, 0x5A


@pytest.fixture(scope="module")
def R(pkg):
    return pkg.COALESCE_TILE   # records per tile of the kernels (kCoalesceTile)


class Buf:
    """`size` bytes on the device at `mis` bytes past an aligned address, guard bytes on both sides."""

    def __init__(self, torch, content: bytes, size: int | None = None, mis: int = 0):
        self.size = len(content) if size is None else size
        self.mis = mis
        self.t = torch.full((GUARD + mis + self.size + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.content = content
        self.torch = torch
        self.fill()
        self.ptr = self.t.data_ptr() + GUARD + mis

    def fill(self):
        self.t.fill_(POISON)
        if self.content:
            lo = GUARD + self.mis
            self.t[lo: lo + len(self.content)].copy_(self.torch.from_numpy(np.frombuffer(self.content, np.uint8).copy()))

    def expect(self, body: bytes, label: str):
        """The whole allocation: guards, then `body`, then POISON up to the size, then guards."""
        assert len(body) <= self.size, label
        want = np.full(self.t.numel(), POISON, np.uint8)
        lo = GUARD + self.mis
        want[lo: lo + len(body)] = np.frombuffer(body, np.uint8)
        got = self.t.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{label}: differs at {(bad[:8] - lo).tolist()} ({bad.size} bytes of {self.size}): "
                                 f"got {got[bad[:8]].tolist()} want {want[bad[:8]].tolist()}")


class DevBatch:
    def __init__(self, torch, spec, mis):
        data, recs, hashes = bytes(spec["data"]), np.ascontiguousarray(spec["recs"], E.RECORD_DTYPE), \
            np.ascontiguousarray(spec["hashes"], np.uint64)
        self.data, self.recs, self.hashes = data, recs, hashes
        self.n_records = len(recs) if spec.get("n_records") is None else spec["n_records"]
        self.max_records = len(recs) if spec.get("max_records") is None else spec["max_records"]
        assert self.max_records <= len(recs) == len(hashes)
        self.cap = E.append_capacity(len(data)) if spec.get("append_cap") is None else spec["append_cap"]
        mb, mr, m8 = mis
        self.bytes = Buf(torch, data, len(data) + self.cap, mb)
        self.d_recs = Buf(torch, recs.tobytes(), None, mr)
        self.d_hashes = Buf(torch, hashes.tobytes() if len(hashes) else bytes(8), None, m8)
        self.d_n = Buf(torch, np.asarray([self.n_records], np.uint64).tobytes(), None, m8)
        self.out = Buf(torch, b"", 8 * self.max_records, mr)
        self.counts = Buf(torch, b"", 32, m8)

    def tuple(self):
        return (self.bytes.ptr if self.bytes.size else 0, len(self.data), self.cap,
                self.d_recs.ptr if self.max_records else 0, self.d_n.ptr, self.max_records, self.d_hashes.ptr,
                self.out.ptr if self.max_records else 0, self.counts.ptr)

    def scrub(self):
        for b in (self.bytes, self.out, self.counts):
            b.fill()

    def check(self, n, slots, label):
        res = E.coalesce(self.data, self.recs, self.hashes, n, slots, self.cap, self.n_records, self.max_records)
        self.counts.expect(res.counts.tobytes(), f"{label}: counts")
        self.out.expect(res.out.tobytes(), f"{label}: records out")
        self.bytes.expect(self.data + res.written, f"{label}: batch and merged text")
        self.d_recs.expect(self.recs.tobytes(), f"{label}: input records")
        self.d_hashes.expect(self.hashes.tobytes() if len(self.hashes) else bytes(8), f"{label}: hashes")
        self.d_n.expect(np.asarray([self.n_records], np.uint64).tobytes(), f"{label}: record count")
        return res


class Dev:
    """A context with the stage open on the test's stream."""

    def __init__(self, pkg, torch, stream, n, slots=16, max_batch=1 << 20):
        self.pkg, self.torch, self.n = pkg, torch, n
        self.slots = slots or E.DEFAULT_SLOTS
        self.r = pkg.Router(n, max_batch)
        self.r.set_stream(stream.cuda_stream)
        self.r.coalesce_open(slots)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.torch.cuda.synchronize()
        self.r.close()

    def upload(self, specs, mis=(0, 0, 0)):
        return [DevBatch(self.torch, dict(zip(("data", "recs", "hashes"), s)) if isinstance(s, tuple) else s, mis)
                for s in specs]

    def check(self, batches, label):
        self.torch.cuda.synchronize()
        return [b.check(self.n, self.slots, f"{label}[{j}]") for j, b in enumerate(batches)]

    def run(self, specs, label, mis=(0, 0, 0)):
        batches = self.upload(specs, mis)
        self.r.coalesce([b.tuple() for b in batches])
        return self.check(batches, label)


def mix(seed, count, n, pool=60):
    """`count` lines: one hot counter, a pool of light ones, other types, and the kinds of unrouted lines."""
    rng = np.random.default_rng(seed)
    lines = []
    for u, k, v in zip(rng.random(count), rng.integers(0, pool, count), rng.integers(-3000, 3000, count)):
        if u < 0.30:
            lines.append(b"hot.x:%d|c" % v)
        elif u < 0.62:
            lines.append(b"svc.req.%d:%d|c" % (k, v))
        elif u < 0.72:
            lines.append(b"svc.req.%d:%d|ms" % (k, abs(v)))
        elif u < 0.80:
            lines.append(b"svc.req.%d:%d|c|@0.5" % (k, abs(v)))
        elif u < 0.84:
            lines.append(b"ab")                       # invalid length
        elif u < 0.88:
            lines.append(b"no colon in this line")    # invalid format
        else:
            lines.append(b"g.%d:%d.5|g" % (k, abs(v)))
    return E.records_of(lines, n)


# ---- record counts and placement ------------------------------------------------------------------------
COUNTS = {"0": (0, 0), "1": (0, 1), "R-1": (1, -1), "R": (1, 0), "R+1": (1, 1), "3R+1": (3, 1)}   # a * R + b


@pytest.mark.parametrize("slots", [16, 0], ids=["16 slots", "default slots"])
@pytest.mark.parametrize("count", list(COUNTS))
def test_record_counts_around_the_tile(pkg, torch_stream, R, count, slots):
    import torch

    k = COUNTS[count][0] * R + COUNTS[count][1]
    with Dev(pkg, torch, torch_stream, 3, slots) as d:
        res, = d.run([mix(7 + k, k, 3)], count)
        assert int(res.counts[0] + res.counts[1]) == k
        if k >= R - 1:
            assert int(res.counts[2]) >= 1 and res.complete


def test_owner_and_members_in_different_tiles_and_workgroups(pkg, torch_stream, R):
    import torch

    lines = [b"filler.%d:1|c" % i for i in range(3 * R + 1)]
    for at, v in ((R - 1, 5), (R, -7), (2 * R + 9, 40), (3 * R, 1000)):
        lines[at] = b"far.apart:%d|c" % v
    for at in (3, R + 3, 2 * R + 3):
        lines[at] = b"other:1|c"
    with Dev(pkg, torch, torch_stream, 4, 0) as d:
        data, recs, hashes = E.records_of(lines, 4)
        res, = d.run([(data, recs, hashes)], "far apart")
        got = [E.line_of(data, res, r) for r in res.out]
        assert got[R - 1] == b"far.apart:1038|c\n" and got[3] == b"other:3|c\n" and int(res.counts[1]) == 5


@pytest.mark.parametrize("count", ["R+1", "3R+1"])
def test_one_name_on_every_line(pkg, torch_stream, R, count):
    import torch

    k = COUNTS[count][0] * R + COUNTS[count][1]
    with Dev(pkg, torch, torch_stream, 4) as d:
        res, = d.run([E.records_of([b"the.one.name:1|c"] * k, 4)], count)
        assert res.counts.tolist() == [1, k - 1, 1, len(b"the.one.name:%d|c\n" % k)]
        assert res.text == b"the.one.name:%d|c\n" % k


def test_every_name_distinct(pkg, torch_stream, R):
    import torch

    lines = [b"test.counter%d:1|c" % i for i in range(2 * R + 17)]
    with Dev(pkg, torch, torch_stream, 3, 0) as d:
        big, = d.run([E.records_of(lines, 3)], "distinct, default slots")
    with Dev(pkg, torch, torch_stream, 3, 16) as d:
        small, = d.run([E.records_of(lines, 3)], "distinct, 16 slots")
    assert big.counts.tolist() == small.counts.tolist() == [len(lines), 0, 0, 0]


# ---- collisions and identity ----------------------------------------------------------------------------
def slot_hash(slot, salt, slots=16):
    """A made-up hash whose slot in a table of `slots` is `slot`."""
    return E.fmix64_inverse(slots * salt + slot)


def test_two_and_three_names_on_one_slot(pkg, torch_stream):
    import torch

    names = [b"first", b"second", b"third", b"alone"]
    hs = [slot_hash(5, 11), slot_hash(5, 12), slot_hash(5, 13), slot_hash(6, 1)]
    order = [0, 1, 2, 0, 3, 1, 2, 3, 0, 1, 1, 2] * 20
    lines = [names[x] + b":%d|c" % (i + 1) for i, x in enumerate(order)]
    data, recs, _ = E.records_of(lines, 1)
    with Dev(pkg, torch, torch_stream, 1) as d:
        res, = d.run([(data, recs, np.array([hs[x] for x in order], np.uint64))], "three names on slot 5")
        first = sum(i + 1 for i, x in enumerate(order) if x == 0)
        alone = sum(i + 1 for i, x in enumerate(order) if x == 3)
        assert res.text == b"first:%d|c\nalone:%d|c\n" % (first, alone)     # the slot's later names stay as they are
        assert int(res.counts[1]) == order.count(0) + order.count(3) - 2
        two = [x for x in order if x != 2]
        lines2 = [names[x] + b":1|c" for x in two]
        data2, recs2, _ = E.records_of(lines2, 1)
        res2, = d.run([(data2, recs2, np.array([hs[x] for x in two], np.uint64))], "two names on slot 5")
        assert res2.text == b"first:%d|c\nalone:%d|c\n" % (two.count(0), two.count(3))


def test_equal_hash_with_other_name_bytes_length_or_route(pkg, torch_stream):
    """sdbm collides: one made-up hash for names that differ in a byte, in their length (one a prefix of the
    other) and for one name under two routes, all inside one wave."""
    import torch

    lines = [b"name.a:1|c", b"name.b:2|c", b"name.a:3|c", b"name.ab:4|c", b"name.a:5|c", b"name.b:6|c", b"name:7|c",
             b"name.a:8|c", b"name.a:9|c"]
    data, recs, _ = E.records_of(lines, 3)
    recs = recs.copy()
    recs["route"] = [1, 1, 1, 1, 1, 1, 1, 2, 1]
    with Dev(pkg, torch, torch_stream, 3) as d:
        res, = d.run([(data, recs, np.full(len(lines), 0xABCDEF, np.uint64))], "one hash")
        assert res.text == b"name.a:18|c\n" and res.counts.tolist() == [6, 3, 1, 12]
        assert [int(r["route"]) for r in res.out] == [1, 1, 1, 1, 1, 2]
        # the same name under two routes, each route with its own hash: two groups
        data2, recs2, _ = E.records_of([b"same.name:1|c"] * 9, 3)
        recs2 = recs2.copy()
        recs2["route"] = [1, 2] * 4 + [1]
        h2 = np.array([slot_hash(3, 1) if x == 1 else slot_hash(4, 1) for x in recs2["route"]], np.uint64)
        res2, = d.run([(data2, recs2, h2)], "two routes")
        assert res2.text == b"same.name:5|c\nsame.name:4|c\n"


# ---- sums ---------------------------------------------------------------------------------------------------
def test_sums_change_digit_count_reach_zero_and_go_negative(pkg, torch_stream, R):
    import torch

    lines = [b"up:999|c", b"up:1|c", b"zero:5|c", b"zero:-5|c", b"neg:3|c", b"neg:-10|c", b"neg:-0|c", b"down:-99|c",
             b"down:-1|c", b"lead:007|c", b"lead:003|c", b"big:999999999|c", b"big:1|c", b"shrink:1000|c", b"shrink:-1|c"]
    with Dev(pkg, torch, torch_stream, 2, 0) as d:
        res, = d.run([E.records_of(lines, 2)], "digit counts")
        assert res.text == (b"up:1000|c\nzero:0|c\nneg:-7|c\ndown:-100|c\nlead:10|c\nbig:1000000000|c\nshrink:999|c\n")
        for v, total in ((999999999, 2 * R * 999999999), (-999999999, -2 * R * 999999999)):
            res, = d.run([E.records_of([b"nine.digits:%d|c" % v] * (2 * R), 2)], f"2R lines of {v}")
            assert res.text == b"nine.digits:%d|c\n" % total and int(res.counts[1]) == 2 * R - 1


# ---- names --------------------------------------------------------------------------------------------------
def test_name_lengths_at_the_limits_and_odd_bytes(pkg, torch_stream):
    import torch

    long_a, long_b, over = b"a" * 1425, b"a" * 1424 + b"b", b"c" * 1426
    lines = [b"x:1|c", long_a + b":5|c", over + b":11|c", b"x:2|c", long_b + b":-999999999|c", long_a + b":6|c",
             over + b":22|c", b"n\x00\xff\x80:1|c", long_b + b":-999999999|c", b"n\x00\xff\x80:2|c", b"n\x00\xff\x81:3|c",
             b"\x00:4|c", b"\x00:5|c"]
    data, recs, hashes = E.records_of(lines, 5)
    with Dev(pkg, torch, torch_stream, 5, 0) as d:
        res, = d.run([(data, recs, hashes)], "names")
        assert res.text == (b"x:3|c\n" + long_a + b":11|c\n" + long_b + b":-1999999998|c\n" + b"n\x00\xff\x80:3|c\n"
                            + b"\x00:9|c\n")
        assert int(res.counts[3]) <= len(data) and max(int(r["length"]) for r in res.out) == 1440
        assert [int(r["length"]) for r in res.out].count(1426 + 6) == 2     # k = 1426 stays unmerged


# ---- hostile records ----------------------------------------------------------------------------------------
def test_hostile_records(pkg, torch_stream, R):
    """Offsets and lengths outside the batch, records that end without a '\\n' or start inside a line, records
    that overlap, every route code and routes past the downstreams: they pass through, and what is a plain counter
    by the bytes it points at is merged as one."""
    import torch

    rng = np.random.default_rng(11)
    data, recs, hashes = mix(5, R + 90, 4)
    recs, hashes = recs.copy(), hashes.copy()
    nb = len(data)
    for i in range(0, len(recs), 3):
        kind = i // 3 % 10
        if kind == 0:
            recs[i]["offset"] = nb - 2
        elif kind == 1:
            recs[i]["offset"] = 0xFFFFFFF0
        elif kind == 2:
            recs[i]["length"] = 0xFFFF
        elif kind == 3:
            recs[i]["length"] = max(int(recs[i]["length"]) - 1, 0)      # no '\n'
        elif kind == 4:
            recs[i]["offset"] += 1                                      # starts inside its line, ends inside the next
        elif kind == 5:
            recs[i]["route"] = int(rng.choice([0xFFFC, 0xFFFD, 0xFFFE, 0xFFFF, 4, 5000]))
        elif kind == 6:
            recs[i] = recs[i - 1]                                       # overlaps its neighbour, with its hash
            hashes[i] = hashes[i - 1]
        elif kind == 7:
            recs[i]["length"] = 0
        elif kind == 8:
            recs[i]["offset"], recs[i]["length"] = nb, 6
        else:
            recs[i]["offset"], recs[i]["length"] = nb - 1, 1
    with Dev(pkg, torch, torch_stream, 4) as d:
        res, = d.run([(data, recs, hashes)], "hostile")
        assert int(res.counts[2]) >= 1
    # overlapping records of one line: the appended bytes may pass nbytes, the cap still holds
    line = b"a:1|c\n"
    many = np.zeros(200, E.RECORD_DTYPE)
    many["length"], many["route"] = 6, 0
    pairs = np.repeat(np.array([E.fmix64_inverse(j) for j in range(100)], np.uint64), 2)   # pair j on slot j
    with Dev(pkg, torch, torch_stream, 4, 4096) as d:
        res, = d.run([(line, many, pairs)], "100 pairs on one line")
        assert int(res.counts[3]) == 600 > len(line) and not res.complete and res.written == b"a:2|c\n"


# ---- device counts and capacities ---------------------------------------------------------------------------
def test_device_count_above_max_records(pkg, torch_stream, R):
    import torch

    data, recs, hashes = mix(3, R + 300, 4)
    with Dev(pkg, torch, torch_stream, 4) as d:
        a, b, c = d.run([dict(data=data, recs=recs, hashes=hashes, n_records=len(recs) + 5000, max_records=R + 9),
                         dict(data=data, recs=recs, hashes=hashes, n_records=17),
                         dict(data=data, recs=recs, hashes=hashes, n_records=1 << 40, max_records=len(recs) - 1)],
                        "clamped counts")
        assert [int(x.counts[0] + x.counts[1]) for x in (a, b, c)] == [R + 9, 17, len(recs) - 1]


@pytest.mark.parametrize("short", [None, "all", 1, 0], ids=["cap 0", "cap exact", "one byte short", "a line short"])
def test_nothing_past_append_cap(pkg, torch_stream, R, short):
    import torch

    data, recs, hashes = mix(21, R + 60, 3)
    total = int(E.coalesce(data, recs, hashes, 3, 16).counts[3])
    first = E.coalesce(data, recs, hashes, 3, 16).out
    cap = {None: 0, "all": total, 1: total - 1, 0: total - 9}[short]
    with Dev(pkg, torch, torch_stream, 3) as d:
        res, = d.run([dict(data=data, recs=recs, hashes=hashes, append_cap=cap)], f"cap {cap} of {total}", mis=(3, 0, 0))
        assert int(res.counts[3]) == total and res.complete == (cap >= total) and len(res.written) == cap
        assert np.array_equal(res.out, first)


# ---- alignment ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mis", [(1, 4, 8), (3, 0, 0), (7, 4, 0), (13, 0, 8), (15, 4, 8)], ids=str)
def test_odd_alignments(pkg, torch_stream, R, mis):
    """The batch at every kind of odd address; records (in and out) at 4 bytes past 8; hashes, the device count
    and the counts at 8 bytes past 16."""
    import torch

    with Dev(pkg, torch, torch_stream, 3) as d:
        res, = d.run([mix(40 + mis[0], R + 33, 3)], f"mis {mis}", mis=mis)
        assert int(res.counts[2]) >= 1


# ---- batches ------------------------------------------------------------------------------------------------
def test_thirty_two_batches_with_empty_ones(pkg, torch_stream, R):
    import torch

    sizes = [0, 1, R + 1, 5, 0, 2 * R, 37, 300] + [11 * (j % 7) for j in range(24)]
    assert len(sizes) == pkg.SR_MAX_BATCHES_PER_LAUNCH
    specs = [dict(zip(("data", "recs", "hashes"), mix(100 + j, s, 6))) for j, s in enumerate(sizes)]
    assert specs[0]["data"] == b""                       # a batch of 0 bytes
    specs[9]["n_records"] = 0                            # records there, the device's count says none
    specs[3]["append_cap"] = 0
    with Dev(pkg, torch, torch_stream, 6) as d:
        res = d.run(specs, "32 batches")
        assert sum(int(x.counts[2]) for x in res) > 20 and res[9].counts.tolist() == [0, 0, 0, 0]
        # one name in every batch: a batch's table is its own
        same = d.run([E.records_of([b"shared:%d|c" % j] * (j + 1), 6) for j in range(32)], "one name in 32 batches")
        assert [x.text for x in same[1:]] == [b"shared:%d|c\n" % (j * (j + 1)) for j in range(1, 32)]


# ---- capture and repeated calls -----------------------------------------------------------------------------
def test_captured_in_a_graph_and_replayed(pkg, torch_stream, R):
    import torch

    with Dev(pkg, torch, torch_stream, 4) as d:
        batches = d.upload([mix(5, R + 40, 4), mix(6, 77, 4)])
        descs = d.r.coalesce_batches([b.tuple() for b in batches])
        d.r.coalesce(descs)            # eager first: the scratch is allocated and the code loaded outside the capture
        d.check(batches, "eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch_stream):
            d.r.coalesce(descs)
        for k in (1, 2):
            for b in batches:
                b.scrub()
            g.replay()
            d.check(batches, f"replay {k}")


def test_tables_are_cleared_between_calls(pkg, torch_stream, R):
    """A second call whose names land on the first call's slots with other owners, and a smaller one after a
    larger one: nothing of an earlier call is seen."""
    import torch

    with Dev(pkg, torch, torch_stream, 2) as d:
        d.run([E.records_of([b"a.a:1|c"] * (R + 5) + [b"b.b:2|c"] * 9, 2)], "first")
        res, = d.run([E.records_of([b"zzz:1|c", b"b.b:2|c", b"a.a:1|c"], 2)], "second")
        assert res.counts.tolist() == [3, 0, 0, 0]
        res, = d.run([E.records_of([b"a.a:4|c", b"q:1|c", b"a.a:-4|c"], 2)], "third")
        assert res.text == b"a.a:0|c\n"


# ---- argument errors ----------------------------------------------------------------------------------------
def test_argument_errors(pkg, torch_stream):
    import torch

    lib, inval = pkg.lib(), -errno.EINVAL
    with pkg.Router(2, 1 << 16) as r:
        r.set_stream(torch_stream.cuda_stream)
        h = r._h
        buf = torch.zeros(1 << 12, dtype=torch.uint8, device="cuda")
        p = buf.data_ptr()
        ok = dict(d_bytes=p, nbytes=64, append_cap=64, d_recs=p + 256, d_n_records=p + 512, max_records=8,
                  d_hashes=p + 1024, d_out=p + 2048, d_counts=p + 3072)
        one = lambda **kw: (pkg.SrCoalesceBatch * 1)(pkg.SrCoalesceBatch(**{**ok, **kw}))
        assert lib.sr_coalesce(h, one(), 1) == inval                          # not open
        for slots in (1, 8, 24, (1 << 22) + 1, 1 << 23):
            assert lib.sr_coalesce_open(h, ctypes.byref(pkg.SrCoalesceConfig(slots))) == inval
        assert lib.sr_coalesce_close(h) == 0                                   # closing a closed stage is fine
        r.coalesce_open(1 << 22)
        assert lib.sr_coalesce_open(h, ctypes.byref(pkg.SrCoalesceConfig(16))) == -errno.EBUSY
        r.coalesce_close()
        r.coalesce_open(16)
        assert lib.sr_coalesce(h, one(), 1) == 0
        assert lib.sr_coalesce(h, None, 1) == inval and lib.sr_coalesce(h, one(), 0) == inval
        assert lib.sr_coalesce(h, (pkg.SrCoalesceBatch * 33)(*[pkg.SrCoalesceBatch(**ok)] * 33), 33) == inval
        for bad in (dict(d_n_records=None), dict(d_counts=None), dict(d_hashes=None), dict(d_bytes=None),
                    dict(d_recs=None), dict(d_out=None), dict(d_out=ok["d_recs"]), dict(d_counts=ok["d_n_records"]),
                    dict(nbytes=(1 << 30) + 1), dict(nbytes=1 << 30, append_cap=0xFFFFFFF0 - (1 << 30) + 1),
                    dict(append_cap=1 << 32), dict(max_records=0xFFFFFFF1)):
            assert lib.sr_coalesce(h, one(**bad), 1) == inval, bad
        # NULL records with no room for any, and NULL bytes with none, are fine
        assert lib.sr_coalesce(h, one(d_recs=None, d_out=None, max_records=0), 1) == 0
        assert lib.sr_coalesce(h, one(d_bytes=None, nbytes=0, append_cap=0), 1) == 0
        torch.cuda.synchronize()
        r.coalesce_close()
        assert lib.sr_coalesce(h, one(), 1) == inval                          # closed again


# ---- composition: route, coalesce, pack, payloads, device resident -------------------------------------------
@pytest.mark.parametrize("dead", [False, True], ids=["alive", "one dead"])
def test_route_coalesce_pack_payloads(pkg, oracle, torch_stream, dead):
    """sr_route_device, sr_coalesce, sr_pack_packets and sr_pack_payloads in a row on device buffers: the packets
    and their bytes equal the restatement's records followed by the oracle's packing of them (what
    tests/pack_records.py and tests/payload_expect.py check the packing stages against)."""
    import torch

    import payload_expect as X

    n = 5
    rng = np.random.default_rng(17)
    lines = [b"e2e.hot:1|c"] * 300 + [b"svc.%d:%d|c" % (i % 23, i) for i in range(400)] + \
            [b"svc.%d:%d|ms" % (i % 5, i) for i in range(50)] + [b"bad", b"nocolon_line"] * 5
    order = rng.permutation(len(lines))
    data = b"".join(lines[i] + b"\n" for i in order)
    alive = None
    if dead:
        recs0, _, _ = oracle.route(np.frombuffer(data, np.uint8), n)
        alive = [1] * n
        alive[int(recs0["route"][recs0["route"] < n][0])] = 0      # a shard that has lines is dead
    fills = rng.integers(1, 1400, n).tolist()
    pending = X.random_pending(rng, fills)
    arr = np.frombuffer(data, np.uint8)
    recs, hashes, n_lines = oracle.route(arr, n, alive)
    cap = E.append_capacity(len(data))
    res = E.coalesce(data, recs, hashes, n, E.DEFAULT_SLOTS, cap)
    assert int(res.counts[2]) >= 20 and res.complete
    whole = np.frombuffer(data + res.text + bytes([0xEE]) * (cap - len(res.text)), np.uint8)

    class Want:
        pass

    e = Want()
    e.probed = oracle.probed_dead(arr, n, alive) if alive is not None else np.zeros(0, np.int64)
    e.sorted, e.packets, e.fill_out, e.n_valid = oracle.pack_packets(res.out, n, fills, e.probed)
    e.n_lines = len(res.out)
    e.pending = dict(pending)
    e.arena, e.offsets, e.rooms = X.flat_expectation(whole, e.sorted, e.packets, e.pending)
    e.flushed, e.new_pending = oracle.materialize(whole, e.sorted, e.packets, e.pending, e.fill_out)
    if dead:
        assert len(e.probed) == 1 and fills[int(e.probed[0])] > 0
    b = X.DeviceBatch(torch, pkg, whole, n, fills, pending, max_records=n_lines)
    b.d_in[len(data):].fill_(0xEE)
    d_hash = torch.zeros(n_lines, dtype=torch.int64, device="cuda")
    d_cout = torch.zeros(n_lines, dtype=torch.int64, device="cuda")
    d_ccnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pkg.Router(n, len(data)) as r:
        if alive is not None:
            r.set_alive(alive)
        r.set_stream(torch_stream.cuda_stream)
        r.coalesce_open()
        r.route_device_many([(b.in_ptr, len(data), b.d_rec.data_ptr(), n_lines, d_hash.data_ptr(), b.d_cnt.data_ptr(),
                              b.d_pd.data_ptr())])
        r.coalesce([(b.in_ptr, len(data), cap, b.d_rec.data_ptr(), b.d_cnt.data_ptr(), n_lines, d_hash.data_ptr(),
                     d_cout.data_ptr(), d_ccnt.data_ptr())])
        r.pack_packets(d_cout.data_ptr(), d_ccnt.data_ptr(), n_lines, b.d_fin.data_ptr(), b.d_pd.data_ptr(),
                       b.d_srt.data_ptr(), b.d_pk.data_ptr(), b.mp, b.d_counts.data_ptr(), b.d_fout.data_ptr())
        r.pack_payloads_many([b.payload_tuple()])
        torch.cuda.synchronize()
        assert d_ccnt.cpu().numpy().view(np.uint64).tolist() == res.counts.tolist()
        assert np.array_equal(d_cout.cpu().numpy().view(E.RECORD_DTYPE)[:len(res.out)], res.out)
        assert np.array_equal(b.d_in.cpu().numpy(), whole)
        X.check(b, e, label=f"route, coalesce, pack, payloads (dead={dead})")
        hot = [p for ps in e.flushed.values() for p in ps if b"e2e.hot:" in p] + \
              [v for v in e.new_pending.values() if b"e2e.hot:" in v]
        assert len(hot) == 1 and hot[0].count(b"e2e.hot:300|c\n") == 1 and hot[0].count(b"e2e.hot:") == 1
