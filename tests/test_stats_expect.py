"""The restatement of the name statistics (tests/stats_expect.py) against what it must hold by construction: the
name hash is the oracle's, the sketch never underestimates, the cardinality estimator stays inside four standard
errors, and the hot set of a fixed input is what the semantics say, overestimates included. CPU only."""
from __future__ import annotations

import math

import numpy as np
import pytest

import stats_expect as E


def test_name_hash_is_the_oracles_with_signed_bytes(pkg, oracle):
    rng = np.random.default_rng(5)
    names = [b"", b"a", b"caf\xc3\xa9.requests", bytes([0x80, 0xFF, 0x7F, 0x00, 0xC3]), b"\xff" * 40]
    for _ in range(40):
        nm = bytes(rng.integers(0, 256, int(rng.integers(1, 60)), dtype=np.uint8)).replace(b":", b";")
        names.append(nm)
    assert any(max(nm, default=0) >= 0x80 for nm in names)
    for nm in names:
        want = oracle.hash_line(nm + b":1|c")
        assert pkg.name_hash(nm) == want == E.name_hash(nm), nm
    assert pkg.name_hash(b"") == 0 == E.fmix64(0)


def test_fmix64_inverse():
    for m in (0, 1, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF, 1 << 63):
        assert E.fmix64(E.fmix64_inverse(m)) == m


def _names_batch(names_with_counts, n=4):
    lines = []
    for nm, k in names_with_counts:
        lines += [nm + b":1|c"] * k
    return E.records_of(lines, n)


def test_sketch_never_underestimates():
    rng = np.random.default_rng(11)
    counts = [(b"n%d" % i, int(rng.integers(1, 40))) for i in range(3000)]
    st = E.Stats(4, dict(hll_p=8, cms_rows=2, cms_width=256, hot_slots=4, hot_div=1, hot_min_lines=1 << 30))
    st.update([_names_batch(counts)])
    snap = st.read()
    over = 0
    for nm, k in counts:
        est = E.estimate(snap, E.name_hash(nm))
        assert est >= k
        over += est > k
    assert over   # 3000 names in 256 cells: collisions are certain, and they only add
    assert snap.total == sum(k for _, k in counts) == int(snap.shard_lines.sum())


@pytest.mark.parametrize("p", [8, 10, 12])
@pytest.mark.parametrize("n", [100, 1000, 20000])
def test_cardinality_within_four_standard_errors(p, n):
    lines = [b"test.counter%d:1|c" % i for i in range(n)]
    st = E.Stats(3, dict(hll_p=p, cms_rows=1, cms_width=256, hot_slots=4, hot_div=1, hot_min_lines=1 << 30))
    st.update([E.records_of(lines, 3)])
    snap = st.read()
    got = E.cardinality(snap)
    bound = 4 * 1.04 / math.sqrt(1 << p)
    print(f"p={p} n={n}: estimate {got:.1f}, relative error {abs(got - n) / n:.4f}, bound {bound:.4f}")
    assert abs(got - n) / n <= bound
    # the shards partition the names: each shard's estimate is inside the same bound of its own count
    for k in range(3):
        own = int(snap.shard_lines[k])
        assert abs(E.cardinality(snap, k) - own) / own <= bound


HOT_INPUT = [(b"svc.req.%d" % i, 1) for i in range(5000)] + [(b"hot.a", 2000), (b"hot.b", 1500), (b"hot.c", 1200)]


def _hot_names(rows, width):
    st = E.Stats(4, dict(hll_p=10, cms_rows=rows, cms_width=width, hot_slots=256, hot_div=16, hot_min_lines=1))
    st.update([_names_batch(HOT_INPUT)])
    snap = st.read()
    assert st.threshold() == -(-9700 // 16) == 607 and not snap.hot_overflow
    return snap, [bytes(e["name"][: e["name_len"]]) for e in snap.hot]


def test_hot_set_is_exactly_the_three_with_the_default_sketch():
    snap, names = _hot_names(4, 4096)
    assert names == [b"hot.a", b"hot.b", b"hot.c"]   # by lines descending
    assert [int(x) for x in snap.hot["lines"]] == [E.estimate(snap, E.name_hash(nm)) for nm in names]
    assert all(int(e["lines"]) >= k for e, k in zip(snap.hot, (2000, 1500, 1200)))


def test_hot_set_of_a_narrow_sketch_includes_a_cold_name_whose_cells_collide():
    snap, names = _hot_names(2, 256)
    assert set(names) >= {b"hot.a", b"hot.b", b"hot.c"}
    cold = [nm for nm in names if nm.startswith(b"svc.req.")]
    print("cold names listed as hot:", cold)
    assert len(names) == 4 and len(cold) == 1   # overestimates are part of the contract
    assert E.estimate(snap, E.name_hash(cold[0])) >= 607
