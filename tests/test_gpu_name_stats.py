"""GPU: sr_stats_update / sr_stats_read, the name statistics kept on the device, against tests/stats_expect.py.
Records and hashes come from the restatement's own tokeniser (names hashed as the oracle hashes them, pinned by
tests/test_stats_expect.py) or are made up, so the stage is driven alone; every snapshot is compared whole:
counters, per-shard sums, every register, every cell, the overflow flag and the hot entries in order."""
from __future__ import annotations

import ctypes
import errno

import numpy as np
import pytest

import stats_expect as E

pytestmark = pytest.mark.gpu

GEN = dict(hll_p=6, cms_rows=3, cms_width=256, hot_slots=16, hot_div=8, hot_min_lines=2)
WIDE = dict(hll_p=8, cms_rows=4, cms_width=4096, hot_slots=8, hot_div=10, hot_min_lines=1)


@pytest.fixture(scope="module")
def R(pkg):
    return pkg.STATS_TILE   # records per tile of the kernels (kStatsTile)


class Dev:
    """A context with the stage open on the test's stream, and the restatement fed the same calls."""

    def __init__(self, pkg, torch, stream, n, cfg=None, max_batch=1 << 20):
        self.pkg, self.torch = pkg, torch
        self.r = pkg.Router(n, max_batch)
        self.r.set_stream(stream.cuda_stream)
        self.r.stats_open(**(cfg or {}))
        self.e = E.Stats(n, cfg)
        self.keep = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.torch.cuda.synchronize()
        self.r.close()

    def _put(self, arr, mis=0):
        raw = np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint8)
        t = self.torch.full((mis + raw.size + 16,), 0x5A, dtype=self.torch.uint8, device="cuda")   # 'Z' around it
        if raw.size:
            t[mis: mis + raw.size].copy_(self.torch.from_numpy(raw.copy()))
        self.keep.append(t)
        return t.data_ptr() + mis, t

    def upload(self, batches, mis=0):
        """batches: (data, records, hashes[, n_records[, max_records]]). The device holds exactly the given
        records; max_records never exceeds them."""
        out = []
        for b in batches:
            data, recs, hashes = bytes(b[0]), np.ascontiguousarray(b[1], dtype=E.RECORD_DTYPE), np.asarray(b[2], np.uint64)
            n_records = b[3] if len(b) > 3 and b[3] is not None else len(recs)
            max_records = b[4] if len(b) > 4 and b[4] is not None else len(recs)
            assert max_records <= len(recs) == len(hashes)
            d_bytes = self._put(np.frombuffer(data, np.uint8), mis)[0] if data else 0
            d_recs = self._put(recs)[0] if len(recs) else 0
            d_hashes = self._put(hashes)[0] if len(recs) else self._put(np.zeros(1, np.uint64))[0]
            d_n = self._put(np.asarray([n_records], np.uint64))[0]
            out.append((d_bytes, len(data), d_recs, d_n, max_records, d_hashes))
        return out

    def update(self, batches, mis=0):
        self.r.stats_update(self.upload(batches, mis))
        self.e.update(batches)

    def check(self, label, overflow_ok=False):
        got, want = self.r.stats_read(), self.e.read()
        bad = E.same(got, want, overflow_ok)
        if bad:
            detail = []
            for f in bad:
                if f in ("lines", "bytes", "shard_lines", "shard_bytes", "regs", "cells"):
                    g, w = np.asarray(getattr(got, f)).ravel(), getattr(want, f).ravel()
                    at = np.flatnonzero(g != w)[:6]
                    detail.append(f"{f}@{at.tolist()}: got {g[at].tolist()} want {w[at].tolist()}")
                elif f == "hot":
                    detail.append(f"hot: got {[(hex(int(e['hash'])), int(e['lines']), int(e['name_len'])) for e in got.hot][:8]} "
                                  f"want {[(hex(int(e['hash'])), int(e['lines']), int(e['name_len'])) for e in want.hot][:8]}")
                else:
                    detail.append(f"{f}: got {getattr(got, f)} want {getattr(want, f)}")
            raise AssertionError(f"{label}: " + "; ".join(detail))
        return got, want


def names_of(snap):
    return [bytes(e["name"][: min(int(e["name_len"]), E.NAME_MAX)]) for e in snap.hot]


def mix(seed, count, n, pool=200, route_of=None):
    """`count` lines: two heavy names, a pool of light ones, and the three kinds of unrouted lines."""
    rng = np.random.default_rng(seed)
    lines = []
    for u, k in zip(rng.random(count), rng.integers(0, pool, count)):
        if u < 0.30:
            lines.append(b"hot.x:1|c")
        elif u < 0.50:
            lines.append(b"hot.y.longer.name:%d|ms" % k)
        elif u < 0.54:
            lines.append(b"ab")                       # invalid length
        elif u < 0.58:
            lines.append(b"no colon in this line")    # invalid format
        else:
            lines.append(b"svc.req.%d:%d|g" % (k, k))
    return E.records_of(lines, n, route_of)


# ---- record counts -----------------------------------------------------------------------------------
COUNTS = {"0": (0, 0), "1": (0, 1), "R-1": (1, -1), "R": (1, 0), "R+1": (1, 1), "3R+1": (3, 1)}   # a * R + b


@pytest.mark.parametrize("count", list(COUNTS))
def test_record_counts_around_the_tile(pkg, torch_stream, R, count):
    import torch

    k = COUNTS[count][0] * R + COUNTS[count][1]
    with Dev(pkg, torch, torch_stream, 3, GEN) as d:
        d.update([mix(7 + k, k, 3)])
        got, want = d.check(count)
        assert want.total + int(want.lines[1:].sum()) == k
        if k > 1000:
            assert {b"hot.x", b"hot.y.longer.name"} <= set(names_of(got)) and not want.hot_overflow


def test_read_before_any_update_and_zero_batches(pkg, torch_stream):
    import torch

    with Dev(pkg, torch, torch_stream, 5) as d:   # the default configuration
        got, _ = d.check("fresh")
        assert got.cfg == pkg.SR_STATS_DEFAULTS
        assert int(got.lines.sum()) == 0 and not got.cells.any() and not got.regs.any() and got.n_hot == 0
        d.update([(b"", np.zeros(0, E.RECORD_DTYPE), np.zeros(0, np.uint64))])
        d.check("an empty batch")


def test_device_count_above_max_records(pkg, torch_stream, R):
    import torch

    data, recs, hashes = mix(3, R + 300, 4)
    with Dev(pkg, torch, torch_stream, 4, GEN) as d:
        d.update([(data, recs, hashes, len(recs) + 5000, R + 9)])     # only max_records are read
        d.update([(data, recs, hashes, 17, None)])                    # only *d_n_records are read
        d.update([(data, recs, hashes, 1 << 40, len(recs) - 1)])
        _, want = d.check("clamped counts")
        assert want.total + int(want.lines[1:].sum()) == R + 9 + 17 + len(recs) - 1


def test_thirty_two_batches_with_empty_ones(pkg, torch_stream, R):
    import torch

    sizes = [0, 1, R + 1, 5, 0, 2 * R, 37, 300] + [11 * (j % 7) for j in range(24)]
    assert len(sizes) == pkg.SR_MAX_BATCHES_PER_LAUNCH
    batches = [mix(100 + j, s, 6) for j, s in enumerate(sizes)]
    batches[9] = batches[9] + (0, None)   # records there, the device's count says none
    with Dev(pkg, torch, torch_stream, 6, GEN) as d:
        d.update(batches)
        got, want = d.check("32 batches")
        assert want.total > 2 * R and b"hot.x" in names_of(got)


# ---- names ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", ["R+1", "3R+1"])
def test_every_line_the_same_name(pkg, torch_stream, R, count):
    import torch

    k = COUNTS[count][0] * R + COUNTS[count][1]
    with Dev(pkg, torch, torch_stream, 4, GEN) as d:
        d.update([E.records_of([b"the.one.name:1|c"] * k, 4)])
        got, _ = d.check(count)
        assert names_of(got) == [b"the.one.name"] and int(got.hot["lines"][0]) == k
        assert pkg.stats_cardinality(got) == pytest.approx(1.0, abs=0.01)


def test_every_name_distinct_beyond_the_sketch(pkg, torch_stream):
    """20000 names: more than the 16384 cells a workgroup's LDS sketch holds; nothing is hot."""
    import torch

    cfg = dict(hll_p=10, cms_rows=4, cms_width=4096, hot_slots=4, hot_div=4, hot_min_lines=1 << 30)
    with Dev(pkg, torch, torch_stream, 3, cfg) as d:
        d.update([E.records_of([b"test.counter%d:1|c" % i for i in range(20000)], 3)])
        got, _ = d.check("20000 distinct names")
        assert abs(pkg.stats_cardinality(got) - 20000) / 20000 <= 4 * 1.04 / 32 and got.n_hot == 0


def test_every_name_distinct_and_hot_beyond_the_workgroup_cache(pkg, torch_stream):
    """3000 names, each hot (T = 1): more than the 256 names a workgroup remembers, all in a 4096-slot table."""
    import torch

    cfg = dict(hll_p=8, cms_rows=2, cms_width=8192, hot_slots=4096, hot_div=1 << 30, hot_min_lines=1)
    lines = [b"n.%d:1|c" % i for i in range(3000)]
    with Dev(pkg, torch, torch_stream, 2, cfg) as d:
        d.update([E.records_of(lines + lines[:700], 2)])
        got, want = d.check("3000 hot names")
        assert got.n_hot == 3000 and not want.hot_overflow and len(set(got.hot["hash"].tolist())) == 3000


def test_the_empty_name(pkg, torch_stream):
    import torch

    with Dev(pkg, torch, torch_stream, 2, GEN) as d:
        d.update([E.records_of([b":12|c"] * 40 + [b"other:1|c"] * 3, 2)])
        got, _ = d.check("empty name")
        assert int(got.hot["hash"][0]) == 0 and int(got.hot["name_len"][0]) == 0 and int(got.hot["lines"][0]) >= 40


# ---- made-up hashes ----------------------------------------------------------------------------------------
def made_up(hashes, n, reps=1, route_of=None):
    """Records over real text whose hashes are the test's own; shard = hash % n unless route_of says."""
    lines = [b"made.up.%d:1|c" % i for i in range(len(hashes))] * reps
    data, recs, _ = E.records_of(lines, max(n, 1))
    hs = np.asarray(list(hashes) * reps, np.uint64)
    recs["route"] = [route_of(int(h)) if route_of else int(h) % n for h in hs]
    return data, recs, hs


@pytest.mark.parametrize("p,rows,width", [(4, 1, 16384), (12, 8, 256), (12, 8, 2048), (4, 1, 256), (10, 4, 4096)])
def test_edge_hashes_in_every_sketch_shape(pkg, torch_stream, p, rows, width):
    """Hash 0, mixed hashes with w == 0 (only register-index bits set), the first and the last register and
    cell; p 4 and 12, one and eight rows, the narrowest and the widest sketch."""
    import torch

    mixed = [0, 1 << (64 - p), ((1 << p) - 1) << (64 - p), 3 << (64 - p),          # w == 0: rho = 64 - p + 1
             1 << 40, 0xFFF00000FFFFFFFF, (0xFFF << 52) | (width - 1), 1, (1 << 64) - 1,
             0x8000000000000000 >> p, (1 << (64 - p)) - 1]
    hashes = [E.fmix64_inverse(m) for m in mixed]
    assert [E.fmix64(h) for h in hashes] == mixed and hashes[0] == 0
    cfg = dict(hll_p=p, cms_rows=rows, cms_width=width, hot_slots=16, hot_div=1 << 20, hot_min_lines=3)
    with Dev(pkg, torch, torch_stream, 3, cfg) as d:
        d.update([made_up(hashes, 3, reps=3)])
        got, want = d.check(f"p={p} D={rows} W={width}")
        assert int(want.regs.max()) == 64 - p + 1 and want.cells[0, 0] >= 3 and want.cells[0, width - 1] >= 3
        assert want.regs[:, 0].any() and want.regs[:, -1].any()
        assert got.n_hot == len(hashes)


# ---- hot names --------------------------------------------------------------------------------------------
def threshold_input():
    lines = [b"at.threshold:1|c"] * 100 + [b"one.below:1|c"] * 99 + [b"single.%d:1|c" % i for i in range(801)]
    return E.records_of(lines, 4)


@pytest.mark.parametrize("hot_min,listed", [(1, [b"at.threshold"]), (100, [b"at.threshold"]), (101, []), (1001, [])])
def test_hot_threshold_is_inclusive_and_gated(pkg, torch_stream, hot_min, listed):
    """1000 lines, hot_div 10: T = max(hot_min_lines, 100). est == T is hot, T - 1 is not; hot_min_lines above
    the estimate or above the total lists nothing."""
    import torch

    with Dev(pkg, torch, torch_stream, 4, dict(WIDE, hot_min_lines=hot_min)) as d:
        d.update([threshold_input()])
        got, want = d.check(f"hot_min_lines={hot_min}")
        assert E.estimate(want, E.name_hash(b"at.threshold")) == 100 and E.estimate(want, E.name_hash(b"one.below")) == 99
        assert d.e.threshold() == max(hot_min, 100) and names_of(got) == listed


def test_hot_over_several_calls(pkg, torch_stream):
    import torch

    singles = lambda a, b: [b"single.%d:1|c" % i for i in range(a, b)]
    with Dev(pkg, torch, torch_stream, 4, WIDE) as d:
        d.update([E.records_of([b"late.riser:1|c"] * 50 + singles(0, 950), 4)])
        got, _ = d.check("first call: 50 of 1000, T = 100")
        assert names_of(got) == []
        d.update([E.records_of([b"late.riser:1|c"] * 150, 4)])
        got, _ = d.check("second call: 200 of 1150, T = 115")
        assert names_of(got) == [b"late.riser"]
        d.update([E.records_of(singles(1000, 6000), 4)])
        got, _ = d.check("third call: diluted, T = 615")
        assert names_of(got) == [b"late.riser"] and int(got.hot["lines"][0]) < d.e.threshold() == 615


def test_hot_table_overflow(pkg, torch_stream):
    import torch

    hot = [b"hot.%d" % i for i in range(6)]
    lines = [nm + b":1|c" for nm in hot for _ in range(150)] + [b"cold.%d:1|c" % i for i in range(100)]
    with Dev(pkg, torch, torch_stream, 4, dict(WIDE, hot_slots=4)) as d:
        d.update([E.records_of(lines, 4)])
        got, want = d.check("six hot names, four slots", overflow_ok=True)
        assert want.hot_overflow == 1 == got.hot_overflow and got.n_hot == 4
        assert set(names_of(got)) <= set(hot) and len(set(got.hot["hash"].tolist())) == 4
        assert [int(x) for x in got.hot["lines"]] == [150] * 4
        assert got.hot["hash"].tolist() == sorted(got.hot["hash"].tolist())   # equal lines: by hash
        for e in got.hot:
            assert int(e["hash"]) == E.name_hash(bytes(e["name"][: e["name_len"]]))


def start_slot(name: bytes, slots: int) -> int:
    """Where stats_hot_insert (csrc/stats_kernel.hpp) starts probing for a name: bits 40.. of the mixed hash."""
    return (E.fmix64(E.name_hash(name)) >> 40) & (slots - 1)


@pytest.mark.parametrize("calls", [1, 2])
def test_full_table_wraps_without_overflow(pkg, torch_stream, calls):
    """Four hot names in four slots, every one of them starting its probe at the LAST slot: whichever is first
    takes it, the other three go on from slot 3 to slots 0, 1 and 2. Nothing overflows, the set is exact. In
    one call they race for the slots; in two calls the second pair finds the first pair settled."""
    import torch

    hot = [b"wrap.1", b"wrap.21", b"wrap.25", b"wrap.29"]
    assert [start_slot(nm, 4) for nm in hot] == [3, 3, 3, 3]   # else the case no longer wraps
    lines = [nm + b":1|c" for nm in hot for _ in range(200)]
    with Dev(pkg, torch, torch_stream, 4, dict(WIDE, hot_slots=4)) as d:
        if calls == 2:
            d.update([E.records_of(lines[:400], 4)])
            got, _ = d.check("the first two names")
            assert sorted(names_of(got)) == hot[:2]
        d.update([E.records_of(lines, 4)])
        got, want = d.check("four names, four slots")
        assert not want.hot_overflow and sorted(names_of(got)) == sorted(hot)


def test_wrapping_probe_skips_other_names(pkg, torch_stream):
    """An eight-slot table: three names that start at slot 7 and two that start at slot 0. The ones from slot 7
    wrap into slots the others want, whoever comes first; all five are listed once."""
    import torch

    pool = [b"wrap.%d" % i for i in range(400)]
    last = [nm for nm in pool if start_slot(nm, 8) == 7][:3]
    first = [nm for nm in pool if start_slot(nm, 8) == 0][:2]
    assert len(last) == 3 and len(first) == 2
    lines = [nm + b":1|c" for nm in last + first for _ in range(150)]
    with Dev(pkg, torch, torch_stream, 3, dict(WIDE, hot_slots=8)) as d:
        d.update([E.records_of(lines, 3)])
        got, want = d.check("five names around the table's end")
        assert not want.hot_overflow and sorted(names_of(got)) == sorted(last + first)


def test_equal_hashes_with_different_routes(pkg, torch_stream, R):
    """Records a route launch cannot produce: one hash under several valid routes, side by side in every wave,
    and runs of one (hash, route) pair between them. Every record counts under its own route: shard sums and
    each shard's registers; the sketch and the hot table know the hash once."""
    import torch

    n = 5
    data, recs, hashes = E.records_of([b"same.hash.everywhere:1|c"] * (R + 70), n)
    i = np.arange(len(recs))
    recs["route"] = np.where(i % 7 < 3, 0, i % n)        # runs of route 0, then routes 2..4 and 0, 1 cycling
    hashes[:] = E.fmix64_inverse(0x0123456789ABCDEF)
    hashes[i % 11 == 5] = E.fmix64_inverse(0xFEDCBA9876543210)
    with Dev(pkg, torch, torch_stream, n, dict(WIDE, hot_div=4)) as d:
        d.update([(data, recs, hashes)])
        got, want = d.check("one hash, five routes")
        assert (want.shard_lines > 0).all() and int((want.regs.max(axis=1) > 0).sum()) == n
        assert got.n_hot >= 1 and int(got.hot["hash"][0]) == E.fmix64_inverse(0x0123456789ABCDEF)


@pytest.mark.parametrize("mis", [0, 1, 3, 7])
def test_names_of_hot_entries(pkg, torch_stream, mis):
    """A 1448-byte name (kept: the first 108 bytes), a name with a NUL and bytes >= 0x80, the last line of the
    buffer, and the batch at odd byte alignments."""
    import torch

    long_name = bytes(65 + (i * 7) % 26 for i in range(1448))
    odd = b"caf\xc3\xa9\x00\xff.\x80x"
    lines = [long_name + b":1|c"] * 30 + [odd + b":1|c"] * 30 + [b"filler.%d:1|c" % i for i in range(20)] + [b"last.line:9|c"] * 30
    data, recs, hashes = E.records_of(lines, 3)
    for i in range(30):   # the router would call these lines too long; the stage follows the records
        hashes[i] = E.name_hash(long_name)
        recs["route"][i] = 1
    with Dev(pkg, torch, torch_stream, 3, dict(WIDE, hot_div=5)) as d:
        d.update([(data, recs, hashes)], mis=mis)
        got, want = d.check(f"names at +{mis}")
        by_len = {int(e["name_len"]): bytes(e["name"]) for e in got.hot}
        assert set(by_len) == {1448, len(odd), 9}
        assert by_len[1448] == long_name[:108] and by_len[len(odd)] == odd + bytes(108 - len(odd))
        assert by_len[9] == b"last.line" + bytes(99)
        assert int(recs["offset"][-1]) + int(recs["length"][-1]) == len(data)


def test_hostile_records(pkg, torch_stream):
    """Routes in [n, 0xFFFD) are ignored; a line reaching past the batch is clipped; a line without ':' is
    its whole clipped run. No byte outside [0, nbytes) is read: the device buffer is followed by 'Z' bytes,
    which would lengthen a name if they were."""
    import torch

    n = 5
    data, recs, hashes = E.records_of([b"real.name:1|c"] * 40 + [b"tail without colon"], n)
    nb = len(data)
    extra = np.zeros(6 * 40, E.RECORD_DTYPE)
    xh = np.zeros(len(extra), np.uint64)
    kinds = [(nb - 8, 300, 0, 0x1111),            # reaches past the end: name = the last 8 bytes (no ':')
             (nb - 19, 19, 1, 0x2222),            # inside, no ':': the whole run
             (nb + 100, 50, 2, 0x3333),           # starts past the end: the empty run
             (0xFFFFFFF0, 0xFFFF, 3, 0x4444),     # offset + length wraps 32 bits
             (0, 20, n, 0x5555),                  # route == n: ignored
             (3, 9, 0xFFFC, 0x6666)]              # the last route below the codes: ignored
    for k, (off, ln, route, h) in enumerate(kinds):
        extra[k::6] = (off, ln, route)
        xh[k::6] = h
    recs, hashes = np.concatenate([recs, extra]), np.concatenate([hashes, xh])
    with Dev(pkg, torch, torch_stream, n, dict(WIDE, hot_div=8)) as d:
        d.update([(data, recs, hashes)], mis=5)
        got, want = d.check("hostile records")
        assert int(want.ignored) == 80 and want.total == 40 + 4 * 40
        names = {int(e["hash"]): bytes(e["name"][: e["name_len"]]) for e in got.hot}
        assert names[0x1111] == data[nb - 8:] and names[0x2222] == b"tail without colon\n"
        assert names[0x3333] == b"" and names[0x4444] == b"" and 0x5555 not in names and 0x6666 not in names
        assert int(want.bytes[0]) == 40 * 14 + 40 * (300 + 19 + 50 + 0xFFFF)


# ---- shards ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 64, 65, 512, 513])
def test_downstream_counts_each_side_of_the_lds_switch(pkg, torch_stream, R, n):
    import torch

    assert pkg.STATS_LDS_SHARDS == 512
    with Dev(pkg, torch, torch_stream, n, GEN) as d:
        spread = lambda h: E.fmix64(h) % n   # sdbm % n alone clusters these names on a few shards
        d.update([mix(n, 2 * R + 77, n, pool=1500, route_of=spread), mix(n + 1, 90, n)])
        _, want = d.check(f"n={n}")
        assert int((want.shard_lines > 0).sum()) >= min(n, 200) and int(want.shard_bytes.sum()) == int(want.bytes[0])


def test_most_downstreams_with_the_smallest_registers(pkg, torch_stream, R):
    import torch

    n = pkg.SR_MAX_DOWNSTREAMS
    hashes = [E.fmix64_inverse(m) for m in range(1, 600)] + [7] * 70
    route_of = lambda h: (h * 40503) % n if h != 7 else n - 1
    with Dev(pkg, torch, torch_stream, n, dict(GEN, hll_p=4)) as d:
        d.update([made_up(hashes, n, reps=2, route_of=route_of)])
        got, want = d.check(f"n={n}, p=4")
        assert int(want.shard_lines[n - 1]) == 140 and got.regs.shape == (n, 16)


def test_no_downstreams(pkg, torch_stream):
    import torch

    with Dev(pkg, torch, torch_stream, 0, GEN) as d:
        d.update([E.records_of([b"name:1|c"] * 30 + [b"x"], 0)])
        _, want = d.check("n=0")
        assert int(want.lines[3]) == 30 and int(want.lines[1]) == 1 and want.total == 0


# ---- calls ------------------------------------------------------------------------------------------------
def test_reset(pkg, torch_stream, R):
    import torch

    with Dev(pkg, torch, torch_stream, 4, GEN) as d:
        d.update([mix(1, R + 5, 4)])
        got, _ = d.check("before the reset")
        assert got.n_hot
        d.r.stats_reset()
        d.e.reset()
        got, _ = d.check("after the reset")
        assert int(got.lines.sum()) == 0 and got.n_hot == 0 and not got.cells.any() and not got.regs.any()
        d.update([mix(2, 300, 4)])
        d.check("counting again")


def test_update_captured_in_a_graph_and_replayed(pkg, torch_stream, R):
    import torch

    batches = [mix(5, R + 40, 4), mix(6, 77, 4)]
    with Dev(pkg, torch, torch_stream, 4, GEN) as d:
        descs = d.r.stats_batches(d.upload(batches))
        d.r.stats_update(descs)        # eager first: the kernels' code is loaded outside the capture
        d.e.update(batches)
        d.check("eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch_stream):
            d.r.stats_update(descs)
        for k in (1, 2):
            g.replay()
            d.e.update(batches)
            _, want = d.check(f"replay {k}")
        assert want.total == 3 * sum(int((b[1]["route"] < 4).sum()) for b in batches)


def test_argument_errors(pkg, torch_stream):
    import torch

    lib, inval = pkg.lib(), -errno.EINVAL
    cfg = lambda **k: ctypes.byref(pkg.SrStatsConfig(**dict(pkg.SR_STATS_DEFAULTS, **k)))
    with pkg.Router(4, 1 << 16) as r:
        r.set_stream(torch_stream.cuda_stream)
        h = r.handle
        one = pkg.SrStatsBatch()
        assert lib.sr_stats_update(h, ctypes.byref(one), 1) == inval       # not open
        assert lib.sr_stats_reset(h) == inval
        p = ctypes.POINTER(pkg.SrStatsSnapshot)()
        assert lib.sr_stats_read(h, ctypes.byref(p)) == inval
        for bad in (dict(hll_p=3), dict(hll_p=13), dict(cms_rows=0), dict(cms_rows=9), dict(cms_width=128),
                    dict(cms_width=768), dict(cms_rows=8, cms_width=4096), dict(hot_slots=2), dict(hot_slots=8192),
                    dict(hot_slots=12), dict(hot_div=0)):
            assert lib.sr_stats_open(h, cfg(**bad)) == inval, bad
        assert lib.sr_stats_open(h, cfg(hll_p=4, cms_rows=1, cms_width=16384, hot_slots=4, hot_div=1, hot_min_lines=0)) == 0
        assert lib.sr_stats_open(h, cfg()) == -errno.EBUSY
        assert lib.sr_stats_close(h) == 0 and lib.sr_stats_open(h, None) == 0     # NULL: the defaults
        buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
        ok = (buf.data_ptr(), 8, buf.data_ptr(), buf.data_ptr() + 32, 2, buf.data_ptr() + 16)
        mk = lambda t: r.stats_batches([t])
        assert lib.sr_stats_update(h, None, 1) == inval
        assert lib.sr_stats_update(h, mk(ok), 0) == inval
        assert lib.sr_stats_update(h, (pkg.SrStatsBatch * 33)(), 33) == inval
        for k in (0, 2, 3, 5):     # d_bytes with bytes, d_recs with records, d_n_records, d_hashes
            t = list(ok)
            t[k] = 0
            assert lib.sr_stats_update(h, mk(tuple(t)), 1) == inval, k
        t = list(ok)
        t[0], t[1], t[2], t[4] = 0, 0, 0, 0     # nothing to read: no pointers needed, but the hashes are
        assert lib.sr_stats_update(h, mk(tuple(t)), 1) == 0
        t[5] = 0
        assert lib.sr_stats_update(h, mk(tuple(t)), 1) == inval
        snap = r.stats_read()
        assert int(snap.lines.sum()) == 0 and snap.cfg == pkg.SR_STATS_DEFAULTS
    with pkg.Router(pkg.SR_MAX_DOWNSTREAMS, 1 << 16) as r:
        assert lib.sr_stats_open(r.handle, cfg(hll_p=11)) == inval   # 65533 << 11 registers: above 2^26
        assert lib.sr_stats_open(r.handle, cfg(hll_p=10)) == 0
