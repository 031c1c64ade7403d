"""The arithmetic behind the route kernel's matrix-core name hash (sdbm_mx, route_kernel.hpp), on the
CPU with numpy: the signed-digit split of K^e mod 2^64, and an integer-matmul model of the
block-diagonal v_mfma_i32_16x16x64_i8 scheme followed by the limb combine, against byte-by-byte sdbm.

Operand layout of the model (what tools/mfma_i8_layout checks on the device): lane l supplies row
(A) / column (B) l & 15; D register r of lane l is row 4 (l >> 4) + r, column l & 15. The 16 bytes of a
lane's fragment sit in k-block l >> 4 in either of the two k orders the probe tests (`contig16`,
`split8`): A and B share the order, and the scheme needs no more than that, so the model runs both."""
from __future__ import annotations

import numpy as np
import pytest

K = 65599
M64 = (1 << 64) - 1


def sdbm(bs):
    """sr-main.c:120-134 over signed chars, u64 wrap."""
    h = 0
    for b in bs:
        c = b - 256 if b >= 128 else b
        h = (h * K + c) & M64
    return h


def digits(v):
    """Eight balanced base-256 digits of v mod 2^64, the carry out of the top digit dropped."""
    out = []
    v &= M64
    for _ in range(8):
        d = v & 0xFF
        if d >= 128:
            d -= 256
        out.append(d)
        v = ((v - d) & M64) >> 8
    return out


KMAPS = {
    "contig16": lambda l, j: 16 * (l >> 4) + j,
    "split8": lambda l, j: 8 * (l >> 4) + j if j < 8 else 32 + 8 * (l >> 4) + j - 8,
}


def mfma_16x16x64(a_frag, b_frag, kmap):
    """D registers [64 lanes][4] of A[16x64] B[64x16] from the lanes' 16-byte fragments (int8)."""
    A = np.zeros((16, 64), np.int64)
    Bm = np.zeros((64, 16), np.int64)
    for l in range(64):
        for j in range(16):
            A[l & 15, kmap(l, j)] = a_frag[l, j]
            Bm[kmap(l, j), l & 15] = b_frag[l, j]
    D = A @ Bm
    assert np.abs(D).max() < 2 ** 31
    return np.array([[D[4 * (l >> 4) + r, l & 15] for r in range(4)] for l in range(64)], dtype=np.int64)


def a_fragments(m, half):
    """The A operand for piece m of a 64-byte window and digits 4 half .. 4 half + 3: lanes on the block
    diagonal ((l >> 4) == (l & 15) >> 2) hold digit 4 half + (l & 3) of K^(63 - 16 m - j), the others 0."""
    a = np.zeros((64, 16), np.int8)
    for l in range(64):
        if (l >> 4) == ((l & 15) >> 2):
            for j in range(16):
                a[l, j] = digits(pow(K, 63 - 16 * m - j, 1 << 64))[4 * half + (l & 3)]
    return a


def combine(s):
    """sum_l S_l 2^(8 l) mod 2^64 the way the kernel does it: pairs in 32 bits, two 64-bit steps, of
    the upper half the low word only."""
    s = [int(x) for x in s]
    p01, p23 = s[0] + (s[1] << 8), s[2] + (s[3] << 8)
    assert abs(p01) < 2 ** 31 and abs(p23) < 2 ** 31
    p45, p67 = (s[4] + (s[5] << 8)) & 0xFFFFFFFF, (s[6] + (s[7] << 8)) & 0xFFFFFFFF
    lo = (p01 + (p23 << 16)) & M64
    hi = (p45 + (p67 << 16)) & 0xFFFFFFFF
    return (lo + (hi << 32)) & M64


def window_values(windows, kmap):
    """V = sum_p b_p K^(63 - p) mod 2^64 of 64 windows of 64 bytes (one per lane) through the model:
    four pieces, two MFMAs each, accumulated; then the limb combine."""
    acc = np.zeros((2, 64, 4), np.int64)
    for m in range(4):
        b = windows[:, 16 * m:16 * m + 16].view(np.int8)
        for half in range(2):
            acc[half] += mfma_16x16x64(A_FRAGS[m][half], b, kmap)
    assert np.abs(acc).max() <= 2 ** 20
    return [combine(list(acc[0, l]) + list(acc[1, l])) for l in range(64)]


A_FRAGS = [[a_fragments(m, half) for half in range(2)] for m in range(4)]
KINV = pow(K, -1, 1 << 64)


def test_digits_reproduce_every_power():
    exps = list(range(64))
    for e in exps:
        v = pow(K, e, 1 << 64)
        d = digits(v)
        assert all(-128 <= x <= 127 for x in d)
        assert sum(x << (8 * i) for i, x in enumerate(d)) & M64 == v, e


def test_inverse_table():
    for z in range(16):
        assert (pow(KINV, z, 1 << 64) * pow(K, z, 1 << 64)) & M64 == 1


@pytest.mark.parametrize("kmap", sorted(KMAPS))
def test_window_model_equals_sdbm(kmap):
    rng = np.random.default_rng(0x5DB)
    w = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    w[0] = 0x80
    w[1] = 0xFF
    w[2, :] = rng.integers(0x80, 0x100, 64, dtype=np.uint8)
    w[3] = 0
    got = window_values(w, KMAPS[kmap])
    for l in range(64):
        assert got[l] == sdbm(w[l].tolist()), l


@pytest.mark.parametrize("kmap", sorted(KMAPS))
def test_pieces_with_zeroed_ends(kmap):
    """One 16-byte piece per lane with every count 0..15 of zeroed leading and trailing bytes (and an
    all-0x80 piece among them): leading zeros are free, z trailing zeros multiply the value by K^z."""
    rng = np.random.default_rng(0x11B5)
    cases = [(lead, trail) for lead in range(16) for trail in range(16) if lead + trail <= 16]
    for c0 in range(0, len(cases), 64):
        chunk = cases[c0:c0 + 64]
        w = np.zeros((64, 64), np.uint8)
        pieces = []
        for l, (lead, trail) in enumerate(chunk):
            p = rng.integers(0, 256, 16, dtype=np.uint8) if l % 3 else np.full(16, 0x80, np.uint8)
            if l % 3 == 1:
                p = rng.integers(0x80, 0x100, 16, dtype=np.uint8)
            p[:lead] = 0
            p[16 - trail:] = 0
            pieces.append((p, lead, trail))
            w[l, 48:] = p   # the window's last piece
        got = window_values(w, KMAPS[kmap])
        for l, (p, lead, trail) in enumerate(pieces):
            name = p[lead:16 - trail].tolist()
            assert got[l] == sdbm(p.tolist())
            assert (got[l] * pow(KINV, trail, 1 << 64)) & M64 == sdbm(name), (lead, trail)


def test_names_over_windows():
    """A name at any start and end mod 16, of any length, over 64-byte windows that end at the name's
    end rounded up to 16 and walk back from there, the way the kernel lays it out:
    h = K^-z sum_k V_k K^(64 k), z = the bytes between the name's end and the last window's."""
    rng = np.random.default_rng(0xA11)
    names = []
    for n in list(range(0, 131)) + [1443]:
        start = int(rng.integers(0, 16)) if n % 16 else n // 16 % 16
        names.append((64 + start, rng.integers(0, 256, n, dtype=np.uint8)))
    wins, meta = [], []
    for start, nm in names:
        end = start + nm.size
        E = (end + 15) & ~15
        nseg = max((E - start + 63) >> 6, 0)
        buf = np.zeros(E + 64 * nseg, np.uint8)
        buf[start:end] = nm
        meta.append((len(wins), nseg, E - end, nm))
        for k in range(nseg):
            lo = E - 64 * (k + 1)
            wins.append(buf[lo:lo + 64] if lo >= 0 else np.concatenate([np.zeros(-lo, np.uint8), buf[:lo + 64]]))
    while len(wins) % 64:
        wins.append(np.zeros(64, np.uint8))
    vals = []
    for i in range(0, len(wins), 64):
        vals += window_values(np.stack(wins[i:i + 64]), KMAPS["contig16"])
    for w0, nseg, z, nm in meta:
        assert 0 <= z < 16
        h = sum(vals[w0 + k] * pow(K, 64 * k, 1 << 64) for k in range(nseg)) & M64
        h = (h * pow(KINV, z, 1 << 64)) & M64
        assert h == sdbm(nm.tolist()), nm.size
