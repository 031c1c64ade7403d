"""The name hash on the matrix cores beyond the every-shard-alive uniform kernel: route_chunk_kernel's U(l)
(sdbm_mx_row; KV_CHUNKS | KV_ALIVE and KV_CHUNKS | KV_DEFER1) and the uniform KV_DEFER1 variant's sdbm_mx,
against the CPU oracle record for record and hash for hash, with sr_last_layout and sr_last_hash_engine
checked after every launch. The KV_DEAD1 variants keep the VALU hash: the same batches through them guard
against anything the two share. Needs an MI355X: `pytest -m gpu`."""
from __future__ import annotations

import numpy as np
import pytest

import byte_streams as B
from test_gpu_sdbm_matrix import COLON_AT, _batch

pytestmark = pytest.mark.gpu

TILE = B.TILE
N = 4
TAIL_RESIDUES = (1, 15, 17, 63)


def _aligned_tile():
    """One tile of 256 back-to-back 64-byte lines (59 name bytes + ':1|c\\n'), the name classes in turn: no
    line crosses a chunk, so the tile takes the path without the block scan, h = K^(c' - 64) (U - Suf)."""
    rng = np.random.default_rng(0xA116)
    classes = ("x80", "xff", "alt", "uniform")
    out = b"".join(B.name_bytes(classes[i % 4], 59, rng) + b":1|c\n" for i in range(TILE // 64))
    assert len(out) == TILE
    return np.frombuffer(out, dtype=np.uint8)


def _tail(r):
    """TILE + 192 + r bytes: the second tile's last 16-byte piece is cut after r % 16 bytes, the lanes
    behind it feed zeros. Its last line (hostile bytes) ends at the batch's last byte and spans the
    chunks of the partial tile; another straddles the tile boundary."""
    rng = np.random.default_rng([0x7A11, r])
    total = TILE + 192 + r
    last = B.name_bytes("x80", 40, rng) + B.uniform_name(rng, 60) + b":" + B.uniform_name(rng, 19) + b"\n"
    return B.place(total, [(TILE - 30, B.name_bytes("xff", 50, rng) + b":1|c\n"), (total - len(last), last)])


@pytest.fixture(scope="module")
def batches():
    """{name: batch}, and the oracle's answer per (name, alive) computed once (expected())."""
    out = {f"sdbm_{v}": _batch(v) for v in sorted(COLON_AT)}
    out["aligned64"] = _aligned_tile()
    out["bytes100"] = B.place(100, [])
    for r in TAIL_RESIDUES:
        out[f"tail_{r}"] = _tail(r)
    return out


@pytest.fixture(scope="module")
def expected(batches, oracle):
    memo = {}

    def get(name, alive):
        key = (name, tuple(alive))
        if key not in memo:
            memo[key] = oracle.route(batches[name], N, list(alive))
        return memo[key]

    return get


def test_batches_hold_what_they_claim(batches, expected):
    recs, _, n = expected("aligned64", (1, 1, 1, 1))
    assert n == TILE // 64 and (recs["length"] == 64).all() and (recs["offset"] % 64 == 0).all() and (recs["route"] < N).all()
    assert batches["bytes100"].size == 100
    for r in TAIL_RESIDUES:
        data = batches[f"tail_{r}"]
        assert data.size == TILE + 192 + r and data[-1] == B.NL
        recs, _, n = expected(f"tail_{r}", (1, 1, 1, 1))
        assert int(recs[-1]["length"]) == 121 and int(recs[-1]["route"]) < N
        assert any(int(x["offset"]) < TILE < int(x["offset"]) + int(x["length"]) and int(x["route"]) < N for x in recs)


ALL, TWO_DEAD, ONE_DEAD = (1, 1, 1, 1), (1, 0, 0, 1), (1, 0, 1, 1)
# (id, layout, alive, want_hashes, matrix engine expected)
CASES = [
    ("chunks_alive", "SR_LAYOUT_CHUNKS", ALL, True, True),
    ("chunks_two_dead", "SR_LAYOUT_CHUNKS", TWO_DEAD, True, True),           # KV_DEFER1
    ("chunks_two_dead_records", "SR_LAYOUT_CHUNKS", TWO_DEAD, False, True),  # ... dhash in the scratch
    ("chunks_one_dead", "SR_LAYOUT_CHUNKS", ONE_DEAD, True, False),          # KV_DEAD1: the guard
    ("uniform_two_dead", "SR_LAYOUT_UNIFORM", TWO_DEAD, True, True),         # KV_PICKS | KV_DEFER1
    ("uniform_one_dead", "SR_LAYOUT_UNIFORM", ONE_DEAD, True, False),
    ("uniform_alive", "SR_LAYOUT_UNIFORM", ALL, True, True),
]
RUNS = [(c, spin) for c in CASES for spin in ((None, 0) if c[1] == "SR_LAYOUT_CHUNKS" else (None,))]


@pytest.mark.parametrize("case,spin", RUNS, ids=[c[0] + ("" if s is None else "_lb_spin0") for c, s in RUNS])
def test_records_hashes_and_engine(pkg, batches, expected, case, spin):
    _, layout, alive, want_hashes, matrix = case
    layout = getattr(pkg, layout)
    engine = pkg.SR_HASH_MATRIX if matrix else pkg.SR_HASH_VALU
    with pkg.Router(N, 2 * TILE + 100) as r:
        r.set_layout(layout)
        r.set_alive(list(alive))
        if spin is not None:   # the look-back fallback: the tail granules q are built from Y, hence from U
            r.set_knob(pkg.SR_KNOB_LB_SPIN, spin)
        for name, data in batches.items():
            gr, gh, gn = r.route(data, want_hashes=want_hashes)
            cr, ch, cn = expected(name, alive)
            assert gn == cn, f"{name}: line count {gn} != {cn}"
            assert np.array_equal(gr, cr), f"{name}: records differ, first at {int(np.nonzero(gr != cr)[0][0])}"
            if want_hashes:
                assert np.array_equal(gh, ch), f"{name}: hashes differ, first at {int(np.nonzero(gh != ch)[0][0])}"
            assert r.last_layout() == layout, name
            assert r.last_hash_engine() == engine, name


def test_engine_is_zero_before_the_first_launch(pkg):
    with pkg.Router(N, TILE) as r:
        assert r.last_hash_engine() == 0
