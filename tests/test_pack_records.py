"""CPU: the record builders of tests/pack_records.py are what they claim, its two references (the
oracle's sro_pack_packets and the plain-Python next_fit written from sr-main.c:73-83) agree on every
batch tests/test_gpu_pack_records.py hands the device, and check_pack notices a result that is wrong
in exactly one place."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import pack_records as R


def _fill_before(lengths, fill, idx):
    """The active buffer's length when line idx arrives (sr-main.c:75-82, on bare lengths)."""
    for L in lengths[:idx]:
        if fill + L > R.CAP:
            fill = 0
        fill += L
    return fill


def _routed_ok(recs, n):
    routed = recs[recs["route"] < n]
    assert routed["length"].min(initial=R.MINL) >= R.MINL and routed["length"].max(initial=R.MINL) <= R.MAXL
    assert len(np.unique(recs["offset"])) == len(recs)
    assert set(recs["route"][recs["route"] >= n].tolist()) <= set(R.UNROUTED)


# ---- builders -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_one_shard(pattern):
    for count in R.COUNTS:
        recs = R.one_shard(count, pattern)
        assert len(recs) == count and (recs["route"] == 1).all()
        _routed_ok(recs, 2)
        assert np.array_equal(recs, R.one_shard(count, pattern))   # seeded
        _, pk, fout, nv = R.next_fit(recs, 2)
        assert nv == count and fout[0] == 0
        closed = pk[pk["open"] == 0]
        if pattern == "six":
            assert (closed["nlines"] == 241).all() and len(pk) == (count + 240) // 241
        if pattern == "max":
            assert (pk["nlines"] == 1).all() and len(pk) == count
        if pattern == "pair":
            assert (closed["nlines"] == 2).all() and (closed["length"] == R.CAP).all()
        if pattern == "alt":
            assert (pk["nlines"] == 1).all() and len(pk) == count
            assert set(recs["length"].tolist()) == ({R.MAXL, 6} if count > 1 else {R.MAXL})
        if pattern == "saw" and count >= R.MAXL - R.MINL + 1:
            assert set(recs["length"].tolist()) == set(range(R.MINL, R.MAXL + 1))
        if pattern == "rand" and count >= 2047:
            assert len(set(recs["length"].tolist())) > 500


@pytest.mark.parametrize("ch", R.CHUNKS)
def test_boundary(ch):
    kinds = set()
    for k in R.BOUNDARY_K:
        x = R.boundary_fill(k)
        L1s = R.boundary_L1(k)
        assert 6 in L1s and R.MAXL in L1s and all(R.MINL <= v <= R.MAXL for v in L1s)
        assert (R.CAP - x in L1s) == (R.MINL <= R.CAP - x) and (R.CAP + 1 - x in L1s) == (R.MINL <= R.CAP + 1 - x)
        for L1 in L1s:
            for at, build in ((1, R.boundary), (2, R.boundary2)):
                recs = build(ch, k, L1, seed=3)
                assert len(recs) == at * ch + 1 + 300 and (recs["route"] == 1).all()
                _routed_ok(recs, 2)
                lens = recs["length"].tolist()
                assert lens[at * ch] == L1 and lens[: at * ch - k] == [R.MAXL] * (at * ch - k)
                assert lens[at * ch - k: at * ch] == [6] * k
                for f in R.BOUNDARY_FILLS:
                    assert _fill_before(lens, f, at * ch) == x, (ch, k, L1, at, f)
                kinds.add("fit" if x + L1 == R.CAP else "over1" if x + L1 == R.CAP + 1 else
                          "full" if k == 0 else "open-six" if L1 == 6 else "other")
    assert {"fit", "over1", "full", "open-six"} <= kinds


def test_skewed():
    n, hot = 65, 64
    recs = R.skewed(n, hot, 500, 3, 0.05, seed=9)
    assert np.array_equal(recs, R.skewed(n, hot, 500, 3, 0.05, seed=9))
    assert not np.array_equal(recs["route"], R.skewed(n, hot, 500, 3, 0.05, seed=10)["route"])
    _routed_ok(recs, n)
    per = np.bincount(recs["route"][recs["route"] < n], minlength=n)
    assert per[hot] == 500 and (np.delete(per, hot) == 3).all()
    un = recs[recs["route"] >= n]
    assert abs(len(un) / len(recs) - 0.05) < 0.002
    assert set(un["route"].tolist()) == set(R.UNROUTED)
    assert {0, 4096} <= set(un["length"].tolist())
    assert (np.diff(recs["route"].astype(np.int64)) != 0).sum() > len(recs) // 4   # shuffled, not grouped
    sparse = R.skewed(n, 3, 3, 3, 0.0, seed=9, every=7)
    per = np.bincount(sparse["route"], minlength=n)
    assert [s for s in range(n) if per[s]] == sorted({3} | set(range(0, n, 7))) and set(per[per > 0]) == {3}


@pytest.mark.parametrize("size", R.UNEVEN_SIZES + (100, 3000, 5000))
def test_mixed(size):
    """Six tenths of about `size` records on one shard, the rest spread evenly, 5 % unrouted from 20 up."""
    n, seed = 16, 97 * 9 + 5
    recs = R.mixed(n, size, seed)
    assert np.array_equal(recs, R.mixed(n, size, seed))
    _routed_ok(recs, n)
    per = np.bincount(recs["route"][recs["route"] < n], minlength=n)
    hot = seed % n
    assert per[hot] == max(1, size * 6 // 10) and (np.delete(per, hot) == (size - per[hot]) // (n - 1)).all()
    routed, un = int(per.sum()), int((recs["route"] >= n).sum())
    assert size - (n - 1) < routed <= size
    assert un == (int(round(0.05 * routed / 0.95)) if size >= 20 else 0)
    assert len(recs) == routed + un and abs(len(recs) - size) <= max(n, size // 15)


@pytest.mark.parametrize("n", R.SHARD_COUNTS)
def test_round_robin(n):
    recs = R.round_robin(n, 3)
    assert len(recs) == 3 * n and np.array_equal(recs["route"], np.arange(3 * n) % n)
    _routed_ok(recs, n)
    rows = recs["route"][: len(recs) // 64 * 64].reshape(-1, 64)
    assert all(len(set(r.tolist())) == 64 for r in rows)


def test_case_lists():
    """What the issue asks of the GPU cases, as conditions on the lists themselves."""
    a = R.cases_counts()
    fills = {}
    for b in a:
        assert b.n == 2 and (b.recs["route"] == 1).all()
        fills.setdefault((len(b.recs), b.name.split("-")[0]), set()).add(int(b.fill[1]))
    assert set(fills) == {(c, p) for c in R.COUNTS for p in R.PATTERNS}
    assert all(len(v) >= 2 and v <= set(R.COUNT_FILLS) for v in fills.values())
    assert {int(b.fill[1]) for b in a} == set(R.COUNT_FILLS) and any(b.fill[0] for b in a)
    for lo in range(0, len(a), 32):   # the batches of one launch differ in size
        assert len({len(b.recs) for b in a[lo: lo + 32]}) >= 10
    for ch in R.CHUNKS:
        b = R.cases_boundary(ch)
        assert len(b) == 16 * 2 * 3 and {int(x.fill[1]) for x in b} == set(R.BOUNDARY_FILLS)
        assert {len(x.recs) for x in b} == {ch + 301, 2 * ch + 301}
    for n in R.SHARD_COUNTS:
        assert R.hot_shards(n)[0] == 0 and R.hot_shards(n)[-1] == n - 1
        assert set(R.hot_shards(n)) >= {s for s in (1023, 1024) if s < n}
        for ch in R.CHUNKS:
            cs = R.cases_shards(n, ch)
            assert len(cs) == 2 * len(R.hot_shards(n)) + 1
            assert max(np.bincount(b.recs["route"][b.recs["route"] < n]).max() for b in cs) == int(2.5 * ch)
            with_lines = without = 0
            for b in cs:
                per = np.bincount(b.recs["route"][b.recs["route"] < n], minlength=n)
                for k in b.probed or ():
                    with_lines += per[k] > 0
                    without += per[k] == 0
            assert with_lines and without and any(b.probed is None for b in cs)
    assert max(len(b.recs) for b in R.cases_shards(4096, 4608)) < 26000
    for nb in R.UNEVEN_BATCHES:
        d = R.cases_uneven(nb)
        assert len(d) == nb and all(b.n == 16 for b in d)
        assert [j for j, b in enumerate(d) if b.null_recs] == sorted({0, 7, 8, nb - 1} & set(range(nb)))
        assert all(b.max_records == 0 and b.lines == 0 for b in d if b.null_recs)
        assert len({tuple(b.fill.tolist()) for b in d}) == nb
    assert 10000 < max(len(b.recs) for b in R.cases_uneven(32)) < 14000
    e = R.cases_capacity()
    assert e["over"].n_records == e["over"].max_records + 1000 and e["over"].lines == e["over"].max_records
    assert e["none"].lines == 0 and e["none"].fill.min() > 0 and e["none"].probed
    assert e["alias"].n == 64 and np.bincount(e["alias"].recs["route"][e["alias"].recs["route"] < 64]).max() > 2 * 2048
    assert [b.max_packets for b in R.capacity_packets(50)] == [0, 1, 49, 50]


# ---- the two references ---------------------------------------------------------------------------
def _all_groups():
    g = {"counts": R.cases_counts, "capacity": lambda: list(R.cases_capacity().values())}
    for ch in R.CHUNKS:
        g[f"boundary-{ch}"] = functools.partial(R.cases_boundary, ch)
        for n in R.SHARD_COUNTS:
            g[f"shards-{n}-{ch}"] = functools.partial(R.cases_shards, n, ch)
    for nb in R.UNEVEN_BATCHES:
        g[f"uneven-{nb}"] = functools.partial(R.cases_uneven, nb)
    return g


GROUPS = _all_groups()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_two_references_agree(oracle, group):
    """next_fit == oracle.pack_packets on every batch of the GPU file, none left out."""
    assert oracle.RECORD_DTYPE == R.RECORD_DTYPE and oracle.PACKET_DTYPE == R.PACKET_DTYPE
    for b in GROUPS[group]():
        srt, pk, fout, nv = R.reference(oracle, b)
        srt2, pk2, fout2, nv2 = b.want(R.next_fit)
        assert nv == nv2 and len(srt) == b.lines, b.name
        assert np.array_equal(srt, srt2), b.name
        assert pk.tobytes() == pk2.tobytes(), b.name
        assert np.array_equal(fout, fout2), b.name
        assert len(pk) <= 2 * b.lines + 5 * b.n + 4
        for k in b.probed or ():
            assert fout[k] == 0


# ---- the checker ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def correct(oracle):
    recs = R.skewed(3, 1, 400, 150, 0.05, seed=21)
    want = oracle.pack_packets(recs, 3, [700, 1449, 3], [2])
    assert len(want[1]) > 100 and want[3] < len(recs)
    return recs, want


def _raw(correct, max_packets=None):
    recs, want = correct
    mp = 2 * len(recs) + 5 * 3 + 4 if max_packets is None else max_packets
    return R.expected_raw(want, len(recs), mp), want, len(recs), mp


def _fails(got, want, mr, mp):
    with pytest.raises(AssertionError):
        R.check_pack(got, want, mr, mp)


def test_check_pack_accepts_a_correct_result(correct):
    R.check_pack(*_raw(correct))
    R.check_pack(*_raw(correct, max_packets=5))
    got, want, mr, _ = _raw(correct, max_packets=0)
    got["packets"] = got["packets"][:0]          # a null d_packets
    R.check_pack(got, want, mr, 0)


def test_check_pack_sees_a_swapped_record(correct):
    got, want, mr, mp = _raw(correct)
    srt = want[0]
    i = next(i for i in range(len(srt) - 1) if srt["route"][i] == srt["route"][i + 1] == 1)
    got["sorted"][[i, i + 1]] = got["sorted"][[i + 1, i]]
    _fails(got, want, mr, mp)


@pytest.mark.parametrize("field", R.PACKET_DTYPE.names)
@pytest.mark.parametrize("delta", (1, -1))
@pytest.mark.parametrize("where", ("first", "middle", "last"))
def test_check_pack_sees_a_packet_field(correct, field, delta, where):
    got, want, mr, mp = _raw(correct)
    k = {"first": 0, "middle": len(want[1]) // 2, "last": len(want[1]) - 1}[where]
    v = got["packets"][field]
    v[k] = (int(v[k]) + delta) % (1 << (8 * v.dtype.itemsize))
    _fails(got, want, mr, mp)


def test_check_pack_sees_fill_and_counts(correct):
    for s in range(3):
        got, want, mr, mp = _raw(correct)
        got["fill_out"][s] ^= 1
        _fails(got, want, mr, mp)
    for c in range(3):
        for delta in (1, -1):
            got, want, mr, mp = _raw(correct)
            got["counts"][c] = int(got["counts"][c]) + delta
            _fails(got, want, mr, mp)


@pytest.mark.parametrize("key", ("sorted", "packets", "counts", "fill_out"))
@pytest.mark.parametrize("max_packets", (None, 5))
def test_check_pack_sees_one_byte_past_an_end(correct, key, max_packets):
    """The first and the last poison byte past each end; with max_packets below the packet count the
    first byte past is a descriptor that must not be written."""
    recs, want = correct
    end = {"sorted": len(recs) * 8, "packets": None, "counts": 3 * 8, "fill_out": 3 * 2}
    for at in ("first", "last"):
        got, want, mr, mp = _raw(correct, max_packets)
        end["packets"] = min(len(want[1]), mp) * 16
        raw = got[key].view(np.uint8).reshape(-1)
        assert raw.size > end[key]
        raw[end[key] if at == "first" else raw.size - 1] ^= 0xFF
        _fails(got, want, mr, mp)


def test_check_pack_sees_an_unwritten_entry(correct):
    """A kernel that skips the last record, the last descriptor or a fill leaves poison there."""
    recs, want = correct
    for key, k in (("sorted", len(recs) - 1), ("packets", len(want[1]) - 1), ("fill_out", 0)):
        got, want, mr, mp = _raw(correct)
        got[key].view(np.uint8).reshape(len(got[key]), got[key].dtype.itemsize)[k] = R.POISON
        _fails(got, want, mr, mp)
