"""Deterministic byte builders for the tests that feed the kernels hostile traffic: names of signed
bytes at every segment and dword edge, lines of every length at every 16-byte alignment, batches at
odd base addresses between poison. A plain helper module (no fixtures, no GPU): every builder has a
fixed seed and returns np.uint8 arrays that end in '\\n'. tests/test_byte_streams.py checks on the CPU,
with the oracle, that the builders are what they claim."""
from __future__ import annotations

import numpy as np

TILE = 16384
MAXL = 1449          # SR_MAX_LINE_LENGTH: the longest valid line, its '\n' included
NL, COLON = 0x0A, 0x3A

NAME_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1447)
NAME_CLASSES = ("x80", "xff", "x7f", "alt", "uniform")
STRADDLE_CLASSES = ("x80", "uniform")
INSIDE_RESIDUES = (1, 2, 3)          # start offsets (mod 4) of the names placed inside a tile

_NO_NL = np.array([b for b in range(256) if b != NL], dtype=np.uint8)
_NAME_POOL = np.array([b for b in range(256) if b not in (NL, COLON)], dtype=np.uint8)


def uniform_name(rng, n):
    """n bytes uniform over everything except '\\n' and ':' (0x00 and every byte >= 0x80 included)."""
    return _NAME_POOL[rng.integers(0, _NAME_POOL.size, n)].tobytes()


def name_bytes(cls, n, rng):
    """n name bytes of one of NAME_CLASSES."""
    if cls == "x80":
        return b"\x80" * n
    if cls == "xff":
        return b"\xff" * n
    if cls == "x7f":
        return b"\x7f" * n
    if cls == "alt":
        return (b"\x80\x7f" * (n // 2 + 1))[:n]
    if cls == "uniform":
        return uniform_name(rng, n)
    raise ValueError(cls)


def name_tail(n):
    """What follows a name of n bytes: ':1|c\\n', or ':\\n' where that would pass 1449 bytes."""
    return b":1|c\n" if n + 5 <= MAXL else b":\n"


def straddle_cuts(n):
    """Name bytes before the tile boundary of the straddling placements of an n-byte name."""
    return sorted({d for d in (1, 17, 64, n - 1) if 1 <= d < n})


def _fill(gap):
    """Exactly `gap` bytes of short lines: valid 8-byte ones, then one that takes the rest."""
    out = bytearray()
    k = 0
    while gap >= 16:
        out += b"f%02d:1|c\n" % (k % 100)
        k += 1
        gap -= 8
    if gap >= 6:
        out += b"g:" + b"7" * (gap - 3) + b"\n"
    elif gap:
        out += b"z" * (gap - 1) + b"\n"
    return bytes(out)


def place(total, placed):
    """A batch of `total` bytes: the (start, bytes) pieces of `placed` at their offsets, short ASCII
    filler lines between them. Every piece ends in '\\n' and so does the batch."""
    out = bytearray()
    for start, piece in sorted(placed):
        assert start >= len(out) and piece[-1] == NL, (start, len(out))
        out += _fill(start - len(out))
        out += piece
    assert len(out) <= total
    out += _fill(total - len(out))
    assert len(out) == total and out[-1] == NL
    return np.frombuffer(bytes(out), dtype=np.uint8)


def extreme_name_cases():
    """{key: 2-tile batch}. Per name class and length of NAME_CLASSES x NAME_LENGTHS:
    `<cls>_<n>_inside`: three lines with such a name inside the second tile, starting at offsets
    = 1, 2, 3 (mod 4); for STRADDLE_CLASSES also `<cls>_<n>_straddle_<d>`: one line whose name has
    exactly d bytes before the boundary at 16384, d in straddle_cuts(n)."""
    rng = np.random.default_rng(0xB17E5)
    cases = {}
    for cls in NAME_CLASSES:
        for n in NAME_LENGTHS:
            tail = name_tail(n)
            cases[f"{cls}_{n}_inside"] = place(2 * TILE, [(TILE + 2000 + 4000 * k + res, name_bytes(cls, n, rng) + tail)
                                                          for k, res in enumerate(INSIDE_RESIDUES)])
            if cls in STRADDLE_CLASSES:
                for d in straddle_cuts(n):
                    cases[f"{cls}_{n}_straddle_{d}"] = place(2 * TILE, [(TILE - d, name_bytes(cls, n, rng) + tail)])
    return cases


def inside_starts():
    """Start offsets of the three names of an `_inside` case."""
    return [TILE + 2000 + 4000 * k + res for k, res in enumerate(INSIDE_RESIDUES)]


# ---- the ragged stream ------------------------------------------------------------------------------

def _valid_line(rng, length):
    """A valid line of `length` bytes ('\\n' included): a uniform name of 1..length-2 bytes, ':', then
    any bytes but '\\n'."""
    assert 6 <= length <= MAXL
    k = int(rng.integers(1, length - 1))            # name bytes, 1 .. length-2
    rest = _NO_NL[rng.integers(0, _NO_NL.size, length - 2 - k)].tobytes()
    return uniform_name(rng, k) + b":" + rest + b"\n"


def _nocolon_line(rng, length):
    return uniform_name(rng, length - 1) + b"\n"


def _invalid_line(rng):
    """No colon (any length 6..1449), 1..5 bytes (with or without a colon), or 1450 / 1451 bytes."""
    k = int(rng.integers(0, 4))
    if k == 0:
        return _nocolon_line(rng, int(rng.integers(6, MAXL + 1)))
    if k == 1:
        return _nocolon_line(rng, int(rng.integers(1, 6)))
    if k == 2:
        L = int(rng.integers(2, 6))
        return b":" + uniform_name(rng, L - 2) + b"\n"
    L = MAXL + 1 + int(rng.integers(0, 2))
    return uniform_name(rng, 3) + b":" + uniform_name(rng, L - 5) + b"\n"


RAGGED_MIN_BYTES = 2 << 20      # what the mandatory content of ragged_stream needs (with room to spare)
WINDOW_RUN = 64                 # consecutive valid 1449-byte lines
EMPTY_RUN = 1100                # consecutive invalid lines (more than two 512-record pack tiles)


def ragged_stream(seed, nbytes):
    """A stream of at most nbytes (>= RAGGED_MIN_BYTES) bytes for the pack kernels:
    - first, for every pair (start mod 16, length mod 16) a valid line with it (a short valid line
      before it moves the start where it has to be), the lengths drawn over the whole 6..1449;
    - then valid lines of every length 6..1449 in a seeded shuffle, more of 16k-1, 16k, 16k+1 and
      1447..1449, and random lengths up to the size asked for; about one line in ten of them is
      followed by an invalid one (no colon; 1..5 bytes; 1450 or 1451 bytes);
    - at seeded places among them: one line of 40 000 and one of 70 000 bytes, a run of WINDOW_RUN valid
      lines of 1449 bytes, a run of EMPTY_RUN invalid lines.
    Name bytes are uniform over everything but '\\n' and ':'."""
    assert nbytes >= RAGGED_MIN_BYTES
    rng = np.random.default_rng([0x7A66ED, seed])
    out = bytearray()
    # every (start, length) residue pair
    for s in range(16):
        for l in range(16):
            pad = (s - len(out)) % 16
            if pad:
                out += _valid_line(rng, pad if pad >= 6 else pad + 16)
            L = l + 16 * int(rng.integers(0, 90))
            if L < 6:
                L += 16
            if L > MAXL:
                L -= 16
            assert len(out) % 16 == s and L % 16 == l
            out += _valid_line(rng, L)
    # every length, the extra ones, and the special runs at seeded places
    lengths = list(range(6, MAXL + 1))
    for k in range(1, MAXL // 16 + 1):
        lengths += [L for L in (16 * k - 1, 16 * k, 16 * k + 1) if 6 <= L <= MAXL]
    lengths += [1447, 1448, 1449] * 8
    lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    specials = {int(p): tag for p, tag in zip(rng.choice(len(lengths), 4, replace=False),
                                              ("long40000", "long70000", "window_run", "empty_run"))}
    for i, L in enumerate(lengths):
        tag = specials.get(i)
        if tag == "long40000":
            out += uniform_name(rng, 100) + b":" + uniform_name(rng, 40000 - 102) + b"\n"
        elif tag == "long70000":
            out += uniform_name(rng, 70000 - 1) + b"\n"
        elif tag == "window_run":
            for _ in range(WINDOW_RUN):
                out += _valid_line(rng, MAXL)
        elif tag == "empty_run":
            for _ in range(EMPTY_RUN):
                out += _nocolon_line(rng, int(rng.integers(1, 6))) if rng.random() < 0.9 else _nocolon_line(rng, 40)
        out += _valid_line(rng, L)
        if rng.random() < 0.1:
            out += _invalid_line(rng)
    assert len(out) <= nbytes, (len(out), nbytes)
    # random lengths up to the size asked for
    while True:
        L = int(rng.integers(6, MAXL + 1))
        line = _valid_line(rng, L)
        if rng.random() < 0.1:
            line += _invalid_line(rng)
        if len(out) + len(line) > nbytes:
            break
        out += line
    return np.frombuffer(bytes(out), dtype=np.uint8)


def cut_at_newline(stream, lo, hi, residue=None, mod=16):
    """The longest prefix of `stream` of lo < size <= hi bytes that ends in '\\n' (and whose size is
    = residue (mod `mod`), if given)."""
    ends = np.nonzero(stream[lo:hi] == NL)[0] + lo + 1
    if residue is not None:
        ends = ends[ends % mod == residue]
    assert ends.size, (lo, hi, residue)
    return stream[: int(ends[-1])]


END_LAST_LENGTHS = (6, 7, 15, 16, 17, 33, 100, 255, 256, 257, 700, 1023, 1024, 1447, 1448, 1449)
END_POISON = b"\xEE"


def end_batches():
    """16 batches whose valid last line ends at the batch's last byte: batch r has nbytes = r (mod 16)
    and a last line of END_LAST_LENGTHS[r] bytes, after a few ragged lines (one of them invalid). No byte
    is END_POISON (drawn ones are replaced by 0xED), so that poison around a batch shows in an output."""
    rng = np.random.default_rng(0xE4D)
    out = []
    for r, last in enumerate(END_LAST_LENGTHS):
        b = bytearray()
        for _ in range(3):
            b += _valid_line(rng, int(rng.integers(6, 400)))
        b += _invalid_line(rng)
        pad = (r - last - len(b)) % 16
        b += _valid_line(rng, pad if pad >= 6 else pad + 16)
        b += _valid_line(rng, last)
        assert len(b) % 16 == r
        a = np.frombuffer(bytes(b), dtype=np.uint8).copy()
        a[a == END_POISON[0]] = 0xED
        out.append(a)
    return out


def embed(batch, lead, poison):
    """(buffer, offset): `batch` between two runs of the repeated `poison` pattern, each of at least
    2 KiB, with offset = `lead` (mod 16): buffer[offset: offset + batch.size] is the batch. The leading
    run is the pattern cut at its front (so any `lead` works with a pattern of any length and the
    byte before the batch is the pattern's last); the trailing run starts with the pattern's first
    byte. In an allocator-aligned device tensor the batch then sits `lead` bytes past a 16-byte
    boundary."""
    assert 0 <= lead < 16 and len(poison) >= 1
    offset = 2048 + lead
    k = (offset + 64) // len(poison) + 1
    run = np.frombuffer(poison * k, dtype=np.uint8)
    buf = np.concatenate([run[run.size - offset:], np.ascontiguousarray(batch, dtype=np.uint8), run[: 2048 + 64]])
    return buf, offset
