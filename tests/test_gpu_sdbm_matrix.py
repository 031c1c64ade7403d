"""The name hash on the matrix cores (sdbm_mx, route_kernel.hpp): route_kernel<256, KV_UNIFORM | KV_ALIVE>
against the CPU oracle, record for record and hash for hash, on batches of two tiles plus a tail
(32 KiB + 100 B) that hold what the 16-byte pieces, the 64-byte windows, the byte masks and the wave-wide
loop can get wrong. The same batches also run with one of four shards dead: that variant keeps the VALU
hash, and the run guards against anything the two accidentally share. Needs an MI355X: `pytest -m gpu`."""
from __future__ import annotations

import numpy as np
import pytest

import byte_streams as B

pytestmark = pytest.mark.gpu

TILE = B.TILE
TOTAL = 2 * TILE + 100
# where the ':' of the line straddling a tile boundary lies, relative to the boundary
COLON_AT = {"before": -10, "last_byte": -1, "on": 0, "after": 10}


def _batch(variant):
    """One batch. Every variant holds: names of every length 1..130 back to back (so their starts walk
    through the offsets mod 16), bytes >= 0x80 in every name class, an empty name, names of 64, 65, 128
    and 1443 bytes, a line without a colon, a 5-byte and a 1450-byte line, and a line straddling each
    of the two tile boundaries with its ':' placed by `variant` (the second boundary gets the next
    placement of COLON_AT)."""
    rng = np.random.default_rng([0x5DB3, sorted(COLON_AT).index(variant)])
    run = bytearray()
    for n in range(1, 131):
        run += B.name_bytes(B.NAME_CLASSES[n % len(B.NAME_CLASSES)], n, rng) + B.name_tail(n)
    run += b":12|c\n" + b":1|c\n" + B.uniform_name(rng, 30) + b"\n"   # empty name; 5 bytes; no colon
    keys = sorted(COLON_AT)
    d1 = COLON_AT[variant]
    d2 = COLON_AT[keys[(keys.index(variant) + 1) % len(keys)]]
    n1, n2 = 100, 70                                   # straddlers' name bytes (two windows each)
    tail = b":" + b"7" * 30 + b"|c\n"                  # ends past the boundary wherever the ':' is
    placed = [
        (0, bytes(run)),
        (TILE + d1 - n1, B.name_bytes("uniform", n1, rng) + tail),
        (TILE + 1003, B.name_bytes("x80", 64, rng) + b":1|c\n" + B.name_bytes("xff", 65, rng) + b":1|c\n" +
         B.name_bytes("alt", 128, rng) + b":1|c\n"),
        (TILE + 2005, B.uniform_name(rng, 1443) + b":1|c\n"),
        (TILE + 4000 + 7, B.uniform_name(rng, 3) + b":" + B.uniform_name(rng, 1445) + b"\n"),   # 1450 bytes
        (TILE + 6000 + 9, B.uniform_name(rng, 1443) + b":1|c\n"),
        (2 * TILE + d2 - n2, B.name_bytes("uniform", n2, rng) + tail),
    ]
    return B.place(TOTAL, placed)


@pytest.fixture(scope="module")
def batches():
    return {v: _batch(v) for v in COLON_AT}


def test_batches_hold_what_they_claim(batches, oracle):
    for v, data in batches.items():
        assert data.size == TOTAL and data[-1] == B.NL
        recs, hs, n = oracle.route(data, 4)
        valid = recs[recs["route"] < 4]
        raw = data.tobytes()
        names = [raw[int(r["offset"]):raw.index(b":", int(r["offset"]))] for r in valid]
        lens = {len(x) for x in names}
        assert set(range(0, 131)) | {1443} <= lens, v
        long_starts = {int(r["offset"]) % 16 for r, x in zip(valid, names) if len(x) > 16}
        assert long_starts == set(range(16)), v
        assert any(b >= 0x80 for x in names for b in x)
        lengths = set(recs["length"].tolist())
        assert {5, 1450} <= lengths
        # the straddlers: a line starts before and ends after each boundary, its ':' where asked
        for bnd in (TILE, 2 * TILE):
            s = raw.rindex(b"\n", 0, bnd - 1) + 1
            c = raw.index(b":", s)
            assert raw.index(b"\n", s) > bnd and c - bnd in COLON_AT.values(), (v, bnd)
        c1 = raw.index(b":", raw.rindex(b"\n", 0, TILE - 1) + 1) - TILE
        assert c1 == COLON_AT[v]


def _same(got, exp, what):
    (gr, gh, gn), (cr, ch, cn) = got, exp
    assert gn == cn, f"{what}: line count {gn} != {cn}"
    assert np.array_equal(gr, cr), f"{what}: records differ, first at {int(np.nonzero(gr != cr)[0][0])}"
    assert np.array_equal(gh, ch), f"{what}: hashes differ, first at {int(np.nonzero(gh != ch)[0][0])}"


@pytest.mark.parametrize("alive", [[1, 1, 1, 1], [1, 0, 1, 1]], ids=["all_alive", "one_dead"])
def test_records_and_hashes_match_the_oracle(pkg, oracle, batches, alive):
    with pkg.Router(4, TOTAL) as r:
        r.set_layout(pkg.SR_LAYOUT_UNIFORM)
        r.set_alive(alive)
        for v, data in batches.items():
            _same(r.route(data, want_hashes=True), oracle.route(data, 4, alive), f"{v} alive={alive}")
            assert r.last_layout() == pkg.SR_LAYOUT_UNIFORM
