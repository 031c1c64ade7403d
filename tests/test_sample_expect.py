"""tests/sample_expect.py against the contract's own examples and invariants (CPU only, no library): the lines that
are sampleable and those that are not, the ladder at every boundary, conservation and the capacity bound on seeded
batches, and the kept share of the keep rule, which must be the share a client's Bernoulli draw would give."""
from __future__ import annotations

import numpy as np
import pytest

import sample_expect as E

C, MS, H, D = 1, 4, 8, 32


@pytest.mark.parametrize("line,want", [
    (b"a:1|c\n", (5, C)), (b"a:1|ms\n", (6, MS)), (b"a:1|h\n", (5, H)), (b"a:1|d\n", (5, D)),
    (b"svc.time:12.5|ms|#env:prod,zone:a\n", (16, MS)), (b"a:1|h|#t:|,:\n", (5, H)), (b"a:b:c|d\n", (7, D)),
    (b"a|b:1|c\n", (7, C)), (b"\x00\xff:\x80|ms\n", (7, MS)), (b"a:-x y|c\n", (8, C)),
    (b"a:1|c|@0.5\n", None), (b"a:1|ms|@1|#t\n", None), (b"a:1|ms|#t|@1\n", (6, MS)),
    (b"a:|ms\n", None), (b"ab:|c\n", None), (b":1|ms\n", None), (b":12|c\n", None),
    (b"a:1|m\n", None), (b"a:1|msx\n", None), (b"a:12|\n", None), (b"a:1||#t\n", None), (b"a:1|g\n", None), (b"a:1|s\n", None),
    (b"a:1|C\n", None), (b"a:1|ms|\n", None), (b"a:1|ms|x\n", None), (b"a:1|ms||#t\n", None), (b"a:1|ms|#\n", (6, MS)),
    (b"a:1|ms", None), (b"ab:1|c", None), (b"abcdef\n", None), (b"abc|c:\n", None), (b"a:123\n", None),
    (b"a:1|\n", None), (b"a:1|c\n"[:5], None), (b"a:1|c\n\n", None),
])
def test_sampleable_lines(line, want):
    assert E.parse(line) == want


def test_the_types_of_the_configuration():
    for line, bit in ((b"a:1|c\n", C), (b"a:1|ms\n", MS), (b"a:1|h\n", H), (b"a:1|d\n", D)):
        for types in range(1, 64):
            if not types & ~E.TYPES_ALL:
                assert (E.parse(line, types) is not None) == bool(types & bit)
    assert E.TYPES_DEFAULT == MS | H | D and E.parse(b"a:1|c\n", E.TYPES_DEFAULT) is None


def test_line_lengths():
    mk = lambda ln: b"a:" + b"1" * (ln - 5) + b"|h\n"
    assert [len(mk(ln)) for ln in (6, 1441, 1442)] == [6, 1441, 1442]
    assert E.parse(b"a:1|c"[:4] + b"\n") is None and len(b"a:1|\n") == 5          # L = 5
    assert E.parse(mk(6)) == (5, H) and E.parse(mk(1441)) == (1440, H) and E.parse(mk(1442)) is None
    assert E.LINE_MAX + E.EXTRA_MAX == 1449 and max(len(r) for r in E.R) + 2 == E.EXTRA_MAX


@pytest.mark.parametrize("limit", [1, 3])
def test_the_ladder_at_every_boundary(limit):
    assert E.step(limit, 0) == 0 and E.step(limit, 1) == 0
    for j, k in enumerate(E.K):
        assert E.step(limit, limit * k) == j
        assert E.step(limit, limit * k + 1) == min(j + 1, E.STEPS - 1)
    assert E.step(limit, limit * 10000 * 1000) == 12 and E.step(limit, (1 << 64) - 1) == 12
    assert len(E.K) == len(E.R) == E.STEPS == 13
    for k, r in zip(E.K[1:], E.R[1:]):
        assert abs(float(r) * k - 1.0) < 1e-12


def seeded(seed, count):
    rng = np.random.default_rng(seed)
    pool = [b"hot.a:%d|ms", b"hot.b:%d|h|#t:v", b"hot.c:%d|c", b"cold.%d:1|d", b"at.a:%d|ms|@0.1", b"bad line %d", b"g.%d:1|g"]
    return E.records_of([pool[k] % rng.integers(0, 1000) for k in rng.integers(0, len(pool), count)], 3)


@pytest.mark.parametrize("seed", range(6))
def test_conservation(seed):
    data, recs, hashes = seeded(seed, 3000)
    res = E.apply(data, recs, hashes, 3, 50 + seed, E.TYPES_ALL, 0, seed)
    out, dropped, rewritten, need = (int(x) for x in res.counts)
    assert out + dropped == len(recs) and out == len(res.out) == len(res.hashes_out) and dropped > 100 and rewritten > 10
    new = res.out[res.out["offset"] >= len(data)]
    assert len(new) == rewritten and int(new["length"].sum()) == need == len(res.text)
    assert int(res.hits[:, 0].sum()) == int((res.steps != E.NOT_SAMPLEABLE).sum())
    assert int(res.hits[:, 1].sum()) == int(res.hits[:, 0].sum()) - dropped and int(res.hits[1:, 1].sum()) == rewritten
    assert need <= E.append_capacity(len(data))
    # every record out names its line: an untouched one, or the input's line with the rate of its step inserted
    kept = np.flatnonzero((res.steps == E.NOT_SAMPLEABLE) | (res.steps & E.DROPPED == 0))
    for i, line in zip(kept, E.lines_of(data, res.text, res.out)):
        o, ln, j = int(recs[i]["offset"]), int(recs[i]["length"]), int(res.steps[i])
        src = data[o:o + ln]
        assert line == (src if j in (0, E.NOT_SAMPLEABLE) else E.rewrite(src, E.parse(src)[0], j))


@pytest.mark.parametrize("count", [1, 2, 3, 6, 11, 1000, 20001])
def test_the_capacity_bound_on_its_worst_family(count):
    """Every line `a:1|c\\n`, the shortest sampleable line, with limit 1: the bound is exact for the longest insert
    on every line, 14 bytes for 6, and whatever is kept stays within it."""
    data, recs, hashes = E.records_of([b"a:1|c"] * count, 2)
    assert count * (6 + E.EXTRA_MAX) == E.append_capacity(len(data))
    for seed in (0, 1):
        res = E.apply(data, recs, hashes, 2, 1, E.TYPES_ALL, 0, seed)
        assert int(res.counts[3]) <= int(res.counts[2]) * (6 + E.EXTRA_MAX) <= E.append_capacity(len(data))
        assert int(res.counts[0] + res.counts[1]) == count


def test_keep_many_is_keep():
    h = E.name_hash(b"api.latency")
    for seed in (0, 1, 0xDEADBEEF, (1 << 64) - 1):
        for j in (0, 1, 5, 12):
            idx = np.concatenate([np.arange(300), [1 << 31, (1 << 32) - 1, (1 << 40) + 5]])
            assert E.keep_many(h, seed, idx, j).tolist() == [E.keep(h, seed, int(i), j) for i in idx]


@pytest.mark.parametrize("k", [2, 5, 10, 100, 1000, 10000])
@pytest.mark.parametrize("seed", [0, 1, 0xDEADBEEF, (1 << 64) - 1])
@pytest.mark.parametrize("name", [b"a", b"api.latency", b"x" * 64])
def test_the_kept_share_of_a_single_name(name, seed, k):
    """200,000 lines of one name at step K: the number kept lies within four standard deviations of c / K (the worst
    of these 72 cases is 2.75)."""
    c = 200000
    kept = int(E.keep_many(E.name_hash(name), seed, np.arange(c), E.K.index(k)).sum())
    sd = (c * (1 / k) * (1 - 1 / k)) ** 0.5
    assert abs(kept - c / k) <= 4 * sd, (kept, c / k, sd)


def test_two_names_interleaved_keep_half_each():
    """Records 0, 2, 4, ... of one name and 1, 3, 5, ... of another at K = 2, 50,000 lines each: the stride of the
    index does not bias the draw. The recorded figures are those of `t.one`'s hash under seed 7 at the even and at
    the odd indices."""
    idx = np.arange(100000)
    sd = (50000 * 0.25) ** 0.5
    for a, b in ((b"t.one", b"t.two"), (b"t.one", b"t.one")):
        even = int(E.keep_many(E.name_hash(a), 7, idx[0::2], 1).sum())
        odd = int(E.keep_many(E.name_hash(b), 7, idx[1::2], 1).sum())
        assert abs(even - 25000) <= 4 * sd and abs(odd - 25000) <= 4 * sd
    assert (even, odd) == (25060, 25112)


def test_specs():
    assert E.parse_spec("4") == (4, MS | H | D) and E.parse_spec("1000:c") == (1000, C)
    assert E.parse_spec("7:ms,h,d,c") == (7, E.TYPES_ALL) and E.parse_spec("4294967295:d,d") == (0xFFFFFFFF, D)
    for bad in ("", "0", "-1", "+4", "4:", "4:x", "4:c,", "4:,c", "4:C", "4 ", " 4", "4:c ms", "4294967296", "4:g", "4:s", "x", "4;c"):
        assert E.parse_spec(bad) is None, bad


def test_configurations():
    for slots in (0, 16, 64, 65536, 1 << 22):
        assert E.check(slots, 1, MS)
    for slots in (1, 8, 15, 17, 48, 1 << 23):
        assert not E.check(slots, 1, MS)
    assert not E.check(0, 0, MS) and not E.check(0, 1, 0) and not E.check(0, 1, 2) and not E.check(0, 1, 16)
    assert not E.check(0, 1, 64) and not E.check(0, 1, MS, 1) and E.check(0, 0xFFFFFFFF, E.TYPES_ALL)
