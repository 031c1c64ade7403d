"""GPU: the MTU packing kernels (mtu_count / mtu_scan / mtu_scatter / mtu_table<2048|4608> / mtu_chain /
mtu_emit<CH, WALK>, through sr_pack_packets and sr_pack_packets_many) on synthetic records, with no
routing in the way: hot and empty shards, both chunk sizes and both chain paths forced by
SR_KNOB_MTU_CHUNK / SR_KNOB_MTU_WALK / SR_KNOB_MTU_XCD, packets placed across line 2048 / 4608 of a
shard, uneven launches and short capacities. Every batch is compared whole with oracle.pack_packets
(sro_pack_packets, the restatement of sr-main.c:49-83) by pack_records.check_pack: counts, sorted
records, descriptors and pending bytes byte for byte, and the poison past every end untouched.
tests/test_pack_records.py checks the inputs, a second reference and the checker on the CPU."""
from __future__ import annotations

import numpy as np
import pytest

import pack_records as R

pytestmark = pytest.mark.gpu

SETTINGS = [(2048, 0), (2048, 1), (4608, 0), (4608, 1)]   # (SR_KNOB_MTU_CHUNK, SR_KNOB_MTU_WALK)


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def _open(pkg, n, chunk=0, walk=1, xcd=1):
    r = pkg.Router(n, 1 << 16)
    r.set_knob(pkg.SR_KNOB_MTU_CHUNK, chunk)
    r.set_knob(pkg.SR_KNOB_MTU_WALK, walk)
    r.set_knob(pkg.SR_KNOB_MTU_XCD, xcd)
    return r


def _check(oracle, b, got):
    try:
        R.check_pack(got, R.reference(oracle, b), b.max_records, b.max_packets)
    except AssertionError as e:
        raise AssertionError(f"batch {b.name!r} ({len(b.recs)} records, n = {b.n}): {e}") from None


def _run(pkg, torch, oracle, router, batches, per=32, single=False):
    """The batches in launches of `per`, each compared with the oracle; returns the raw results."""
    out = []
    for lo in range(0, len(batches), per):
        part = batches[lo: lo + per]
        got = R.run_pack(pkg, torch, router, part, single=single)
        for b, g in zip(part, got):
            _check(oracle, b, g)
        out += got
    print(f"{len(batches)} batches compared in {(len(batches) + per - 1) // per} launches")
    return out


@pytest.mark.parametrize("chunk,walk", SETTINGS)
def test_counts_at_the_chunk_sizes(pkg, oracle, torch, chunk, walk):
    """(a) one shard of 1 .. 9217 lines in six length patterns, from six fills; shard 0 empty, its
    fill passed through. 32 batches of different sizes per launch."""
    with _open(pkg, 2, chunk, walk) as r:
        _run(pkg, torch, oracle, r, R.cases_counts())


@pytest.mark.parametrize("chunk,walk", SETTINGS)
def test_packets_across_a_chunk_boundary(pkg, oracle, torch, chunk, walk):
    """(b) at line ch and 2 ch of a shard (ch the forced chunk size): the exact fit, the overflow by
    one (the chunk's first line opens a packet), a full buffer, a packet of sixes open across it."""
    with _open(pkg, 2, chunk, walk) as r:
        _run(pkg, torch, oracle, r, R.cases_boundary(chunk))


# walk has no effect above 64 shards (mtu_chain always): both values at n = 64 only
SHARD_SETTINGS = [(c, 1, n) for c in (0, 2048, 4608) for n in R.SHARD_COUNTS] + [(c, 0, 64) for c in (0, 2048, 4608)]


@pytest.mark.parametrize("chunk,walk,n", SHARD_SETTINGS)
def test_many_shards_skew_and_chain(pkg, oracle, torch, chunk, walk, n):
    """(c) a hot shard of 2.5 chunks at shard 0, n - 1 and the slice edges of the 1024-thread kernels
    among shards of three lines; mostly empty shards; round robin; random fills; probed-dead bits on
    shards with and without lines (fill_out 0). The heuristic (chunk 0) picks 2048 lines at these sizes."""
    batches = R.cases_shards(n, chunk or 2048)
    with _open(pkg, n, chunk, walk) as r:
        _run(pkg, torch, oracle, r, batches, per=R.per_call(n))


@pytest.mark.parametrize("xcd", (0, 1))
def test_uneven_launches(pkg, oracle, torch, xcd):
    """(d) 8, 9, 31 and 32 batches of 0 .. ~12 k records in one launch, empty batches (max_records 0,
    null record pointers) first, at index 7, at index 8 and last; with and without the per-XCD deal of
    the chunks (eight batches or more)."""
    with _open(pkg, 16, xcd=xcd) as r:
        for nb in R.UNEVEN_BATCHES:
            _run(pkg, torch, oracle, r, R.cases_uneven(nb))


def test_more_records_than_capacity(pkg, oracle, torch):
    """(e) *d_n_records = max_records + 1000: the first max_records are packed."""
    b = R.cases_capacity()["over"]
    with _open(pkg, b.n) as r:
        (g,) = _run(pkg, torch, oracle, r, [b])
    assert int(g["counts"][2]) == b.max_records == len(b.recs) - 1000


def test_descriptor_capacity(pkg, oracle, torch):
    """(e) max_packets in {0 with a null d_packets, 1, npk - 1, npk}: the count is the full number and
    nothing past max_packets is written."""
    npk = len(R.reference(oracle, R.cases_capacity()["shape"])[1])
    assert npk > 1000
    batches = R.capacity_packets(npk)
    with _open(pkg, batches[0].n) as r:
        got = _run(pkg, torch, oracle, r, batches)
    assert [int(g["counts"][0]) for g in got] == [npk] * 4
    assert [len(g["packets"]) for g in got] == [0, 1 + R.EXTRA, npk - 1 + R.EXTRA, npk + R.EXTRA]


def test_no_records(pkg, oracle, torch):
    """(e) *d_n_records = 0 with fills and probed bits: the fills pass through, the probed ones drop."""
    b = R.cases_capacity()["none"]
    with _open(pkg, b.n) as r:
        (g,) = _run(pkg, torch, oracle, r, [b])
    want = [0 if k in b.probed else int(f) for k, f in enumerate(b.fill)]
    assert g["fill_out"][: b.n].tolist() == want and [int(c) for c in g["counts"][:3]] == [0, 0, 0]


def test_single_equals_many_of_one(pkg, oracle, torch):
    """(e) sr_pack_packets and sr_pack_packets_many of one batch leave the same bytes."""
    b = R.cases_capacity()["shape"]
    with _open(pkg, b.n) as r:
        (one,) = _run(pkg, torch, oracle, r, [b], single=True)
        (many,) = _run(pkg, torch, oracle, r, [b])
    for key in ("sorted", "packets", "counts", "fill_out"):
        assert one[key].tobytes() == many[key].tobytes(), key


def test_fill_in_place_at_64_shards(pkg, oracle, torch):
    """(e) d_fill_out aliasing d_fill_in with a multi-chunk shard at n = 64: the launch drops the emit
    kernel's walk for mtu_chain, which reads every fill before it writes one."""
    b = R.cases_capacity()["alias"]
    assert np.bincount(b.recs["route"][b.recs["route"] < b.n]).max() > 2 * 2048
    with _open(pkg, b.n) as r:
        _run(pkg, torch, oracle, r, [b])
