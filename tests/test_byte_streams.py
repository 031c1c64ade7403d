"""CPU: the builders of tests/byte_streams.py are what they claim, measured with the oracle's own line
split and verdicts. These are conditions on the inputs of the GPU tests in test_gpu_route_variants.py
and test_gpu_pack_bytes.py, which therefore never skip or filter a case."""
from __future__ import annotations

import numpy as np
import pytest

import byte_streams as B

RAGGED_BYTES = 3 << 20
INVALID_FROM = 0xFFFD          # SR_ROUTE_INVALID_LENGTH: the smallest route code that is no shard


@pytest.fixture(scope="module")
def ragged():
    return B.ragged_stream(1, RAGGED_BYTES)


@pytest.fixture(scope="module")
def ragged_recs(ragged, oracle):
    recs, _, n = oracle.route(ragged, 1)
    assert n == len(recs)
    return recs


def _class_ok(cls, name):
    a = np.frombuffer(name, dtype=np.uint8)
    if cls == "x80":
        return bool((a == 0x80).all())
    if cls == "xff":
        return bool((a == 0xFF).all())
    if cls == "x7f":
        return bool((a == 0x7F).all())
    if cls == "alt":
        return bool((a[0::2] == 0x80).all() and (a[1::2] == 0x7F).all())
    return bool(((a != B.NL) & (a != B.COLON)).all())


def test_extreme_name_cases(oracle):
    cases = B.extreme_name_cases()
    assert B.extreme_name_cases().keys() == cases.keys()
    assert all(np.array_equal(v, B.extreme_name_cases()[k]) for k, v in list(cases.items())[:5])   # seeded
    seen_zero = False
    for cls in B.NAME_CLASSES:
        for n in B.NAME_LENGTHS:
            v = cases.pop(f"{cls}_{n}_inside")
            assert v.size == 2 * B.TILE and v[-1] == B.NL
            recs, _, _ = oracle.route(v, 1)
            raw = v.tobytes()
            by_start = {int(r["offset"]): r for r in recs}
            for start, res in zip(B.inside_starts(), B.INSIDE_RESIDUES):
                assert start % 4 == res and start // B.TILE == (start + n + 5) // B.TILE == 1
                r = by_start[start]
                assert int(r["route"]) == 0 and int(r["length"]) == n + len(B.name_tail(n)) <= B.MAXL
                line = raw[start: start + int(r["length"])]
                assert line.index(b":") == n and line[n:] == B.name_tail(n) and _class_ok(cls, line[:n])
                seen_zero |= cls == "uniform" and 0 in line[:n]
            if cls not in B.STRADDLE_CLASSES:
                continue
            cuts = B.straddle_cuts(n)
            assert set(cuts) == {d for d in (1, 17, 64, n - 1) if 0 < d < n}
            for d in cuts:
                v = cases.pop(f"{cls}_{n}_straddle_{d}")
                assert v.size == 2 * B.TILE and v[-1] == B.NL
                recs, _, _ = oracle.route(v, 1)
                off, ln = recs["offset"].astype(np.int64), recs["length"].astype(np.int64)
                over = np.nonzero((off < B.TILE) & (off + ln > B.TILE))[0]
                assert over.size == 1
                r = recs[int(over[0])]
                start = int(r["offset"])
                line = v.tobytes()[start: start + int(r["length"])]
                assert B.TILE - start == d, "name bytes before the boundary"
                assert int(r["route"]) == 0 and line.index(b":") == n and _class_ok(cls, line[:n])
    assert not cases, f"cases nobody asked for: {sorted(cases)}"
    assert seen_zero, "the uniform class never drew 0x00"
    assert 1447 + len(B.name_tail(1447)) == B.MAXL


def test_ragged_ends_and_is_seeded(ragged):
    assert ragged[-1] == B.NL and B.RAGGED_MIN_BYTES <= ragged.size <= RAGGED_BYTES
    assert ragged.size > RAGGED_BYTES - 2 * B.MAXL - 4
    assert np.array_equal(ragged, B.ragged_stream(1, RAGGED_BYTES))
    assert not np.array_equal(ragged[:4096], B.ragged_stream(2, RAGGED_BYTES)[:4096])
    assert (ragged >= 0x80).mean() > 0.4 and (ragged == 0).any()


def test_ragged_lengths_and_residue_pairs(ragged_recs):
    valid = ragged_recs[ragged_recs["route"] < INVALID_FROM]
    lens = valid["length"].astype(np.int64)
    count = np.bincount(lens, minlength=B.MAXL + 1)
    assert count[:6].sum() == 0 and lens.max() == B.MAXL
    missing = [L for L in range(6, B.MAXL + 1) if count[L] == 0]
    assert not missing, f"valid lengths never drawn: {missing}"
    for k in range(1, B.MAXL // 16 + 1):
        assert all(count[L] >= 2 for L in (16 * k - 1, 16 * k, 16 * k + 1) if 6 <= L <= B.MAXL), k
    assert all(count[L] >= 9 for L in (1447, 1448, 1449))
    pairs = set(zip((valid["offset"] % 16).tolist(), (lens % 16).tolist()))
    assert len(pairs) == 256, f"(start, length) residues missing: {sorted(set((s, l) for s in range(16) for l in range(16)) - pairs)}"
    # the prefix the base-alignment test routes (three tiles) already holds hostile bytes in every pair's line
    first = valid[valid["offset"] < 3 * B.TILE]
    assert len(set(zip((first["offset"] % 16).tolist(), (first["length"].astype(np.int64) % 16).tolist()))) >= 32


def test_ragged_invalid_lines_and_runs(ragged, ragged_recs):
    route = ragged_recs["route"]
    lens = ragged_recs["length"].astype(np.int64)
    bad = route >= INVALID_FROM
    # the kinds of invalid line
    assert ((route == 0xFFFE) & (lens >= 6) & (lens <= B.MAXL)).sum() >= 20          # no colon
    assert all(((lens == L) & bad).any() for L in (1, 2, 3, 4, 5, 1450, 1451))
    assert (lens[bad & (lens <= 5)] > 0).all()
    assert (lens == 40000).sum() == 1 and (lens == 0xFFFF).sum() == 1               # the 70 000-byte line saturates
    starts = ragged_recs["offset"].astype(np.int64)
    true_len = np.diff(np.concatenate([starts, [ragged.size]]))
    assert sorted(true_len[true_len > 1451].tolist()) == [40000, 70000]
    # about one in ten outside the empty run
    frac = (bad.sum() - B.EMPTY_RUN) / len(route)
    assert 0.05 < frac < 0.15, frac

    def longest_run(mask):
        edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
        return int((edges[1::2] - edges[0::2]).max()) if edges.size else 0

    assert longest_run((~bad) & (lens == B.MAXL)) >= B.WINDOW_RUN >= 64
    assert longest_run(bad) >= B.EMPTY_RUN >= 256
    # the window run's pieces: 64 lines of 91 16-byte pieces are several windows of 1024 pieces
    assert B.WINDOW_RUN * ((B.MAXL + 15) // 16) >= 5 * 1024


def test_cut_at_newline(ragged):
    for res in (0, 1, 5, 15):
        p = B.cut_at_newline(ragged, 2 * B.TILE, 3 * B.TILE, res)
        assert 2 * B.TILE < p.size <= 3 * B.TILE and p.size % 16 == res and p[-1] == B.NL
        assert np.array_equal(p, ragged[: p.size])
    for res in range(4):
        p = B.cut_at_newline(ragged, 500_000, 600_000, res, mod=4)
        assert p.size % 4 == res and p[-1] == B.NL


def test_end_batches(oracle):
    bs = B.end_batches()
    assert len(bs) == 16 and sorted(B.END_LAST_LENGTHS)[0] == 6 and sorted(B.END_LAST_LENGTHS)[-1] == B.MAXL
    for r, b in enumerate(bs):
        recs, _, n = oracle.route(b, 1)
        last = recs[-1]
        assert b[-1] == B.NL and b.size % 16 == r and not (b == B.END_POISON[0]).any() and (b >= 0x80).any()
        assert int(last["route"]) == 0 and int(last["length"]) == B.END_LAST_LENGTHS[r]
        assert int(last["offset"]) + int(last["length"]) == b.size
        assert (recs["route"] >= INVALID_FROM).any()


def test_probed_dead_signed_fixture_matches_oracle(oracle):
    """tests/golden/probed_dead_signed.json (the compiled reference's own drop while it routed the
    signed-name fixture, written by make_golden.py) against the oracle's restatement; and the fixture
    holds what it was made for."""
    import json
    import os

    from conftest import GOLDEN, load_case

    want = json.load(open(os.path.join(GOLDEN, "probed_dead_signed.json")))
    assert list(want) == ["signed_long_names_n5"]
    c = load_case("signed_long_names_n5")
    n = c["n"]
    alive = [int((int(c["alive"][k >> 6]) >> (k & 63)) & 1) for k in range(n)]
    assert (n, alive) == (5, [1, 0, 1, 1, 1])
    assert all(len(d) <= 4095 for d in c["dgrams"])
    framed = b"".join(oracle.frame(d) for d in c["dgrams"])
    assert oracle.probed_dead(framed, n, alive).tolist() == want["signed_long_names_n5"] == [1]
    # valid lines with a name of each length whose every byte is >= 0x80
    recs = c["records"]
    names = {}
    for r in recs[recs["route"] < INVALID_FROM]:
        line = framed[int(r["offset"]): int(r["offset"]) + int(r["length"])]
        name = line[: line.index(b":")]
        if name and min(name) >= 0x80:
            names.setdefault(len(name), set()).add(name[:1])
    assert set(B.NAME_LENGTHS) <= set(names)
    assert all({b"\x80", b"\xff"} <= names[k] for k in B.NAME_LENGTHS)
    assert (recs["route"] == 0xFFFD).sum() >= 2 and not (recs["route"] == 1).any()


@pytest.mark.parametrize("poison", [b"\n:", b"\xEE", b"abc"])
def test_embed(poison):
    batch = np.frombuffer(b"name:1|c\nx\n", dtype=np.uint8)
    for lead in range(16):
        buf, off = B.embed(batch, lead, poison)
        assert off % 16 == lead and off >= 2048 and buf.size - off - batch.size >= 2048
        assert np.array_equal(buf[off: off + batch.size], batch)
        want = np.frombuffer(poison * (buf.size // len(poison) + 1), dtype=np.uint8)
        assert np.array_equal(buf[:off][::-1], want[: (off // len(poison) + 1) * len(poison)][::-1][:off])
        assert np.array_equal(buf[off + batch.size:], want[: buf.size - off - batch.size])
