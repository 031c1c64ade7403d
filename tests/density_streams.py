"""Batches built tile by tile for the route kernel's lanes-per-line group size G: every full 16 KiB
tile holds a chosen number of '\\n' bytes, so the kernel picks a chosen G for it (expected_G), and the
names inside are what the hash over G lanes can get wrong: every (start, end) alignment mod 16, lengths at
the 16-byte piece and 64-byte window edges and at 64 G, bytes >= 0x80 in names and right around them, long
names beside short, invalid and empty ones in one wave, lines straddling tile boundaries. A plain helper
module (no fixtures, no GPU): every builder has a fixed seed and returns np.uint8 arrays that end in
'\\n'. tests/test_density_streams.py checks on the CPU, with the oracle, that the builders are what they
claim.

A tile's line count is set with the lengths of the values after the ':' (any bytes but '\\n', the first
and last three >= 0x80), with short valid lines of 0..15 name bytes, and, where bytes are left over, with
one invalid line (no colon, or 1450 bytes and up) that ends the tile."""
from __future__ import annotations

import numpy as np

import byte_streams as B

TILE, MAXL, NL, COLON = B.TILE, B.MAXL, B.NL, B.COLON
MAX_NAME = MAXL - 2             # the longest name of a valid line: name, ':', '\n'
_VALUE_POOL = np.array([b for b in range(256) if b != NL], dtype=np.uint8)   # value bytes: anything but the line end
WIN = 256                       # lines a tile stages and hashes per round (SmemT::kWin, route_kernel.hpp)
GROUPS = (1, 2, 4, 8, 16, 32)
# '\n' bytes per tile for which the kernel picks each G (the table of expected_G)
COUNT_RANGE = {32: (1, 15), 16: (16, 31), 8: (32, 63), 4: (64, 127), 2: (128, 252), 1: (253, TILE)}
# per G, the '\n' counts its tiles cycle through (both edges of the range among them)
TILE_COUNTS = {32: (15, 13, 15, 11, 15, 14), 16: (31, 24, 17, 31, 20), 8: (63, 50, 33, 63, 40),
               4: (127, 100, 65, 127, 80), 2: (252, 200, 129, 252, 160), 1: (253, 257, 256, 512, 300, 254, 400, 255)}
THRESHOLD_COUNTS = (15, 16, 31, 32, 63, 64, 127, 128, 252, 253, 256, 257)
SCENARIO_LONG = 1420            # a name of the most windows (23) whose line can still grow by 15 bytes
TAIL_RESIDUE = 5                # batch size mod 16


def expected_G(tile_count):
    """Lanes per line of a tile with tile_count '\\n' bytes (> 0). Mirrors route_kernel.hpp, route_kernel,
    "lanes per line from the mean line length":
        int G = 1;
        while (G < 32 && (G * 64 + 1) * (int)tile_count <= kTileB) G <<= 1;
    A property of the builders below, not an observation of the device: if the kernel's rule changes,
    this changes with it."""
    assert tile_count > 0
    G = 1
    while G < 32 and (G * 64 + 1) * tile_count <= TILE:
        G <<= 1
    return G


def edge_lengths(G):
    """The name lengths the alignment grid deals round-robin: piece and window edges, 64 G and 128 G."""
    raw = (0, 1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 127, 128, 129, 64 * G - 1, 64 * G, 64 * G + 1, 128 * G + 1,
           1023, 1024, 1025, 1443, 1447)
    out = []
    for n in raw:
        if n <= MAX_NAME and n not in out:
            out.append(n)
    return out


def grid_names(G, rng):
    """256 (name, start mod 16) pairs, one per (start, end) residue pair: the lengths of edge_lengths(G)
    round-robin, each moved by less than 16 to hit its pair, the name classes rotating against them."""
    lens = edge_lengths(G)
    out = []
    for i in range(256):
        a, b = i >> 4, i & 15
        n0 = lens[i % len(lens)]
        n = n0 + (b - a - n0) % 16
        if n > MAX_NAME:
            n -= 16
        assert abs(n - n0) < 16 and (a + n) % 16 == b
        cls = B.NAME_CLASSES[(i + i // len(lens)) % len(B.NAME_CLASSES)]
        out.append((B.name_bytes(cls, n, rng), a))
    return out


class _V:
    """A valid line: name, ':', vlen value bytes, '\\n'. res: wanted start mod 16 (None: any)."""

    def __init__(self, name, res=None):
        self.name, self.res = name, res
        self.vlen = max(min(3, MAX_NAME - len(name)), 4 - len(name), 0)
        self.nl = 1

    def size(self):
        return len(self.name) + 2 + self.vlen

    def room(self):
        return MAXL - self.size()

    def bytes(self, rng):
        v = _VALUE_POOL[rng.integers(0, _VALUE_POOL.size, self.vlen)].copy()
        v[:3] |= 0x80
        v[-3:] |= 0x80
        return self.name + b":" + v.tobytes() + b"\n"


class _R:
    """Given bytes that end in '\\n' (invalid lines)."""

    res = None

    def __init__(self, raw):
        assert raw[-1] == NL
        self.raw, self.nl = raw, raw.count(b"\n")

    def size(self):
        return len(self.raw)

    def room(self):
        return 0

    def bytes(self, rng):
        return self.raw


# straddlers: (bytes of the line before the boundary, name bytes, name class, line bytes)
STRADDLERS = (
    (1448, 1440, "uniform", MAXL),      # starts 1448 bytes before the boundary, its '\n' the first byte after
    (151, 150, "x80", 175),             # ':' on the last byte before the boundary
    (100, 100, "alt", 130),             # ':' on the first byte after it
    (70, 200, "uniform", 240),          # the name's first 70 bytes before the boundary
    (1000, 1300, "xff", 1320),          # ... and 1000 of 1300
)


class _Batch:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.out = bytearray()
        self.counts = []        # '\n' bytes of every full tile
        self.turn = 0

    def short(self):
        """A short valid line: 0..15 name bytes of rotating class."""
        self.turn += 1
        return _V(B.name_bytes(B.NAME_CLASSES[self.turn % 5], (7 * self.turn) % 16, self.rng))

    def tile(self, count, head=(), grid=None, straddle=None):
        """The next full tile, with exactly `count` '\\n' bytes in it: the lines of `head` first (no line is
        put between them), then lines from the front of `grid` while bytes and line count allow, short valid
        lines up to the count, the bytes left over spread over the values, and one invalid line up to the
        boundary, or up to the start of the straddling line if one is asked for (its '\\n' counts for the
        next tile)."""
        rng, out = self.rng, self.out
        t = len(out) // TILE
        carry = 1 if len(out) % TILE else 0      # the '\n' of the line straddling into this tile
        assert not (head and carry)
        end = (t + 1) * TILE - (straddle[0] if straddle else 0)
        lines, pos, k = [], len(out), carry

        def push(item, glued=False):
            nonlocal pos, k
            if item.res is not None and pos % 16 != item.res:
                delta = (item.res - pos) % 16
                if lines and isinstance(lines[-1], _V) and lines[-1].room() >= delta:
                    lines[-1].vlen += delta
                    pos += delta
                else:   # a short line of the length that moves the start there
                    assert not glued
                    al = _V(b"k")
                    al.vlen += (item.res - pos - al.size()) % 16
                    lines.append(al)
                    pos += al.size()
                    k += 1
            lines.append(item)
            pos += item.size()
            k += item.nl

        for item in head:
            push(item, glued=True)
        while grid:
            name, res = grid[0]
            item = _V(name, res)
            left = count - k - 3                 # lines still to come after an aligner, this one and the last
            if left < 0 or pos + 21 + item.size() + 24 * left + 1 > end:
                break
            push(item)
            grid.pop(0)
        extra = count - k - 1
        assert extra >= 0, (count, k)
        for _ in range(extra):
            push(self.short())
        assert end - pos >= 1, (count, end - pos)
        # the bytes left over: 16 at a time into the values (alignments stay), the rest to the last line
        units = (end - pos - 1) // 16
        flex = [x for x in lines if isinstance(x, _V)]
        while units:
            share = max(1, units // max(len(flex), 1))
            gave = 0
            for x in flex:
                g = min(share, x.room() // 16, units)
                x.vlen += 16 * g
                units -= g
                gave += g
            if not gave:
                break
        pos = len(out) + sum(x.size() for x in lines)
        rest = end - pos
        if rest >= MAXL + 1 and t % 2:           # 1450 bytes and up, with a colon
            last = B.uniform_name(rng, 3) + b":" + B.uniform_name(rng, rest - 5) + b"\n"
        else:                                    # no colon, any length
            last = B.uniform_name(rng, rest - 1) + b"\n"
        for x in lines:
            out += x.bytes(rng)
        out += last
        assert len(out) == end
        if straddle:
            d, n, cls, size = straddle
            assert d < size <= MAXL and n + 2 <= size
            out += B.name_bytes(cls, n, rng) + b":" + B.uniform_name(rng, size - n - 2) + b"\n"
        self.counts.append(count)

    def tail(self):
        """The short partial tile: valid lines, under 200 bytes, the batch size = TAIL_RESIDUE (mod 16)."""
        assert len(self.out) % TILE == 0
        rng = self.rng
        for cls, n in (("x80", 20), ("uniform", 40), ("xff", 2), ("alt", 17)):
            self.out += _V(B.name_bytes(cls, n, rng)).bytes(rng)
        last = _V(B.name_bytes("uniform", 33, rng))
        last.vlen += (TAIL_RESIDUE - len(self.out) - last.size()) % 16
        self.out += last.bytes(rng)
        assert len(self.out) % 16 == TAIL_RESIDUE and len(self.out) % TILE < 200

    def array(self):
        assert self.out[-1] == NL
        return np.frombuffer(bytes(self.out), dtype=np.uint8)


def _heads(G, which, rng):
    """The lines that open a scenario tile: whole waves (64 / G lines each) of
    - a name of the most windows there are beside one that fits a single 16-byte piece,
    - names of 1..16 bytes only,
    - a multi-window name beside an invalid line and an empty name (with two lines to a wave, G = 32,
      beside ':1|c', which is both; then beside a valid empty name; then beside a line without a colon)."""
    lpw = 64 // G
    cls = B.NAME_CLASSES[which:] + B.NAME_CLASSES[:which]
    mixed = (3, 17, 5, 64, 9, 2, 33, 12, 70, 1)
    nocolon = B.uniform_name(rng, 30) + b"\n"

    def fill(wave):
        i = 0
        while len(wave) < lpw:
            wave.append(_V(B.name_bytes(cls[i % 5], mixed[(i + which) % len(mixed)], rng)))
            i += 1
        assert len(wave) == lpw
        return wave

    a = fill([_V(B.name_bytes(cls[0], SCENARIO_LONG, rng)), _V(B.name_bytes(cls[1], 3 + which, rng), res=4 + which)])
    b = [_V(B.name_bytes(cls[i % 5], 1 + (5 * i + which) % 16, rng)) for i in range(lpw)]
    multi = 200 + 64 * which
    if G == 32:
        c = [_V(B.name_bytes(cls[2], multi, rng)), _R(b":1|c\n"),
             _V(B.name_bytes(cls[3], multi + 1, rng)), _V(b""),
             _V(B.name_bytes(cls[4], multi + 2, rng)), _R(nocolon)]
    else:
        c = [_V(B.name_bytes(cls[2], multi, rng)), _R(nocolon), _R(b":1|c\n"), _V(b"")]
        i = 0
        while len(c) < lpw:
            c.append(_V(B.name_bytes(cls[i % 5], 1 + (3 * i) % 12, rng)))
            i += 1
    return a + b + c


def density_batch(G):
    """One batch whose every full tile holds a '\\n' count for which the kernel picks G lanes per line
    (COUNT_RANGE[G]), and a short partial tile. Tiles in order: a scenario tile (_heads), five tiles that
    end in the lines of STRADDLERS, a tile at the low edge of the range, the second scenario tile, then
    tiles at TILE_COUNTS[G] until the 256 lines of the alignment grid (grid_names) are placed; grid lines
    fill every tile that has room."""
    assert G in GROUPS
    b = _Batch([0xDE45, G])
    grid = grid_names(G, b.rng)
    counts = TILE_COUNTS[G]
    lo, hi = COUNT_RANGE[G]
    b.tile(counts[0], head=_heads(G, 0, b.rng), grid=grid)
    for i, s in enumerate(STRADDLERS):
        b.tile(counts[(i + 1) % len(counts)], grid=grid, straddle=s)
    b.tile(counts[0], grid=grid)                 # takes the last straddler's '\n'
    b.tile(lo, grid=grid)
    b.tile(counts[0], head=_heads(G, 1, b.rng), grid=grid)
    i = 0
    while grid:
        b.tile(counts[i % len(counts)], grid=grid)
        i += 1
    assert all(lo <= c <= hi and expected_G(c) == G for c in b.counts)
    b.tail()
    return b.array()


def threshold_batch():
    """Consecutive tiles of exactly THRESHOLD_COUNTS '\\n' bytes (where G flips, and the edge of the 256-line
    staging window), each with names of 129 bytes and more that hold bytes >= 0x80 and start off a 16-byte
    boundary; two of the boundaries are straddled; a short partial tile."""
    b = _Batch([0xDE45, 0])
    for i, count in enumerate(THRESHOLD_COUNTS):
        G = expected_G(count)
        grid = [(B.name_bytes(("x80", "xff", "alt")[i % 3], 129 + 7 * i, b.rng), 1 + i % 15),
                (B.name_bytes(("alt", "x80", "xff")[i % 3], min(64 * G + 1, MAX_NAME), b.rng), 1 + (i + 5) % 15),
                (b"\x80" + B.uniform_name(b.rng, 300 + i), 1 + (i + 9) % 15)]
        b.tile(count, grid=grid, straddle={3: STRADDLERS[3], 8: STRADDLERS[1]}.get(i))
        assert not grid
    assert tuple(b.counts) == THRESHOLD_COUNTS
    b.tail()
    return b.array()


def all_batches():
    """{name: batch}: density_batch(G) as "G<G>" for every G, and threshold_batch() as "threshold"."""
    out = {f"G{G}": density_batch(G) for G in GROUPS}
    out["threshold"] = threshold_batch()
    return out
