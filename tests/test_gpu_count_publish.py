"""The tile's early count publish (tile_load, route_kernel.hpp): in route_kernel<256, KV_UNIFORM | KV_ALIVE>
each wave adds its '\\n' count to one LDS word as soon as it has it, and the wave that arrives fourth stores
the tile's status granule, ahead of the workgroup barrier. The smallest shapes at which that can go wrong,
through the C ABI, record for record, hash for hash and count for count against the CPU oracle
(oracle/sr_oracle.route), the outputs prefilled with a sentinel.

| stream | what it holds |
|---|---|
| `one_16384`, `one_16385`, `one_100` | one tile exactly, a second tile of one byte, a 100-byte batch |
| `wave0` .. `wave3` | a middle tile whose '\\n' bytes all lie in one wave's 4 KiB: three waves add zero |
| `no_newline` | a middle tile without a '\\n' (a line longer than the tile): count 0, its neighbours still get bases |
| `straddle` | three tiles, a line across each boundary, its ':' before the first and after the second |
| `six_byte` | tiles of 6-byte lines: more than 256 lines per tile, so the restage path runs |
| `u1` | 40/70/100/130-byte lines over two tiles: unaligned name windows, partial pieces at every z |

Launches of 7, 9 and 32 batches cover the non-class path, the XCD classes, padding blocks and scanners; the
same launch three times eagerly and three times from a captured graph covers the epoch advance and the LDS
word, which starts fresh per workgroup; shard counts 1, 3, 4, 5, 16, 17 and 64 cover both sides of the shard
pick. Needs an MI355X: `pytest -m gpu`."""
from __future__ import annotations

import numpy as np
import pytest

import byte_streams as B
from test_gpu_route_variants import SLACK, _Launch

pytestmark = pytest.mark.gpu

TILE = B.TILE
WAVE = TILE // 4
SHARDS = (1, 3, 4, 5, 16, 17, 64)


def _long(n, colon_at):
    """A line of n bytes ('\\n' included) with its ':' at byte colon_at."""
    assert 0 < colon_at < n - 1
    return b"n" * colon_at + b":" + b"7" * (n - colon_at - 2) + b"\n"


def _one_wave(w):
    """Three tiles; the '\\n' bytes of tile 1 all lie in wave w's 4 KiB of it."""
    lo, hi = TILE + WAVE * w + 100, TILE + WAVE * (w + 1) - 200
    first = _long(lo - (TILE - 50), 40)                  # ends at byte lo - 1, in wave w
    last = _long(2 * TILE + 77 - hi, 60)                 # starts in wave w, ends in tile 2
    return B.place(3 * TILE, [(TILE - 50, first), (hi, last)])


def _six_byte(total):
    out = bytearray()
    k = 0
    while len(out) + 6 <= total:
        out += bytes([97 + k % 26]) + b":" + bytes([48 + k % 10]) + b"|c\n"
        k += 1
    out += B._fill(total - len(out)) if total - len(out) else b""
    return np.frombuffer(bytes(out), dtype=np.uint8)


@pytest.fixture(scope="module")
def streams(pkg):
    s = {
        "one_16384": B.place(TILE, []),
        "one_16385": B.place(TILE + 1, []),
        "one_100": B.place(100, []),
        "no_newline": B.place(4 * TILE, [(TILE - 30, _long(TILE + 60, 20))]),
        "straddle": B.place(3 * TILE, [(TILE - 60, _long(100, 30)), (2 * TILE - 40, _long(100, 70))]),
        "six_byte": _six_byte(2 * TILE + 1000),
        "u1": pkg.gen_stream(2 * TILE, [40, 70, 100, 130], seed=0x5EED0141).data.copy(),
    }
    for w in range(4):
        s[f"wave{w}"] = _one_wave(w)
    return s


@pytest.fixture(scope="module")
def dev(streams):
    import torch

    return {k: torch.from_numpy(v.copy()).to("cuda") for k, v in streams.items()}


@pytest.fixture(scope="module")
def expected(streams, oracle):
    """(stream, N) -> (records, hashes, count, no probed-dead shard) of the oracle, computed once."""
    memo = {}

    def get(name, n=4):
        if (name, n) not in memo:
            memo[(name, n)] = oracle.route(streams[name], n) + ([],)
        return memo[(name, n)]

    return get


def test_streams_hold_what_they_claim(streams):
    nl = {k: np.flatnonzero(v == B.NL) for k, v in streams.items()}
    assert [streams[k].size for k in ("one_16384", "one_16385", "one_100")] == [TILE, TILE + 1, 100]
    assert all(v[-1] == B.NL for v in streams.values())
    for w in range(4):
        p = nl[f"wave{w}"]
        mid = p[(p >= TILE) & (p < 2 * TILE)]
        assert mid.size > 100 and mid.min() >= TILE + WAVE * w and mid.max() < TILE + WAVE * (w + 1)
    p = nl["no_newline"]
    assert not ((p >= TILE) & (p < 2 * TILE)).any() and (p < TILE).any() and (p >= 2 * TILE).sum() > 1000
    raw = streams["straddle"].tobytes()
    for bnd, side in ((TILE, -1), (2 * TILE, 1)):
        s = raw.rindex(b"\n", 0, bnd - 1) + 1
        assert raw.index(b"\n", s) > bnd and (raw.index(b":", s) - bnd) * side > 0
    p = nl["six_byte"]
    assert (p < TILE).sum() > 2 * 256 and np.all(np.diff(p[:2000]) == 6)
    lens = set(np.diff(nl["u1"]).tolist())
    assert lens == {40, 70, 100, 130} and streams["u1"].size > TILE + 130


def _route_one(pkg, r, n, d_in, size, exp, what):
    m = _Launch(pkg, n, [d_in], [size], [exp[2] + SLACK])
    r.route_device_many(m.descs)
    assert r.last_layout() == pkg.SR_LAYOUT_UNIFORM and r.last_hash_engine() == pkg.SR_HASH_MATRIX
    m.check([exp], what)


@pytest.mark.parametrize("name", ["one_16384", "one_16385", "one_100", "wave0", "wave1", "wave2", "wave3",
                                  "no_newline", "straddle", "six_byte", "u1"])
def test_each_stream_alone(pkg, streams, dev, expected, torch_stream, name):
    size = int(streams[name].size)
    with pkg.Router(4, size) as r:
        r.set_layout(pkg.SR_LAYOUT_UNIFORM)
        r.set_stream(torch_stream.cuda_stream)
        _route_one(pkg, r, 4, dev[name], size, expected(name), name)


@pytest.mark.parametrize("n", SHARDS)
def test_shard_counts(pkg, streams, dev, expected, torch_stream, n):
    """Powers of two and their neighbours: both sides of the shard pick, on the unaligned stream."""
    size = int(streams["u1"].size)
    with pkg.Router(n, size) as r:
        r.set_layout(pkg.SR_LAYOUT_UNIFORM)
        r.set_stream(torch_stream.cuda_stream)
        _route_one(pkg, r, n, dev["u1"], size, expected("u1", n), f"u1 N={n}")


def _many(streams, nb):
    """nb batches of one or two tiles (and the odd sizes between), every stream used."""
    small = ["one_16384", "u1", "one_16385", "six_byte", "one_100"]
    names = [small[i % len(small)] for i in range(nb)]
    names[nb // 2] = "wave2"            # three tiles among them: the classes are unbalanced (padding blocks)
    return names


@pytest.mark.parametrize("nb", [7, 9, 32])
def test_many_batches_one_launch(pkg, streams, dev, expected, torch_stream, nb):
    names = _many(streams, nb)
    exp = [expected(k) for k in names]
    sizes = [int(streams[k].size) for k in names]
    with pkg.Router(4, max(sizes)) as r:
        r.set_layout(pkg.SR_LAYOUT_UNIFORM)
        r.set_stream(torch_stream.cuda_stream)
        m = _Launch(pkg, 4, [dev[k] for k in names], sizes, [e[2] + SLACK for e in exp])
        r.route_device_many(m.descs)
        assert r.last_hash_engine() == pkg.SR_HASH_MATRIX
        m.check(exp, f"{nb} batches")


def test_repeated_launches_and_graph_replays(pkg, streams, dev, expected, torch_stream):
    """The same launch three times eagerly, then three replays of its capture, outputs cleared between."""
    import torch

    names = _many(streams, 9) + ["no_newline", "straddle"]
    exp = [expected(k) for k in names]
    sizes = [int(streams[k].size) for k in names]
    with pkg.Router(4, max(sizes)) as r:
        r.set_layout(pkg.SR_LAYOUT_UNIFORM)
        r.set_stream(torch_stream.cuda_stream)
        m = _Launch(pkg, 4, [dev[k] for k in names], sizes, [e[2] + SLACK for e in exp])
        for i in range(3):
            m.clear()
            r.route_device_many(m.descs)
            m.check(exp, f"eager launch {i}")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch_stream):
            r.route_device_many(m.descs)
        for i in range(3):
            m.clear()
            g.replay()
            m.check(exp, f"graph replay {i}")
