"""The every-shard-alive uniform route kernel in its shape for eight workgroups per CU (route_kernel.hpp,
kOcc8): a 1536-byte halo, 16-bit line ends and first colons, the power tables in the image's pad
dwords. Batches of two to four 16 KiB tiles, built byte by byte around what those cuts can break,
against the CPU oracle: records and hashes bit for bit, every shard alive (N = 4 and 16), uniform
layout. Needs an MI355X: `pytest -m gpu`."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 16384
MAXL = 1449          # SR_MAX_LINE_LENGTH: the longest valid line, its '\n' included
SHARDS = (4, 16)


def _name(rng, n):
    """n name bytes, a third of them >= 0x80 (the sdbm takes signed chars), none '\\n' or ':'."""
    lo = rng.integers(0x21, 0x7F, n, dtype=np.uint8)
    hi = rng.integers(0x80, 0x100, n, dtype=np.uint8)
    b = np.where(rng.random(n) < 0.33, hi, lo).astype(np.uint8)
    b[b == ord(":")] = ord("a")
    return b.tobytes()


def _line(rng, length, colon_at=None):
    """A line of `length` bytes, '\\n' included; colon_at: index of its only ':' (None: no colon)."""
    body = bytearray(_name(rng, length - 1))
    if colon_at is not None:
        body[colon_at] = ord(":")
    return bytes(body) + b"\n"


def _fill(rng, gap):
    """Exactly `gap` bytes of short lines (valid 8-byte ones, then one that takes the rest)."""
    out = bytearray()
    while gap >= 16:
        out += _line(rng, 8, 3)
        gap -= 8
    if gap >= 6:
        out += _line(rng, gap, 1)
    elif gap:
        out += b"z" * (gap - 1) + b"\n"
    return bytes(out)


def _place(rng, total, placed):
    """A batch of `total` bytes: the (start, bytes) pieces of `placed` at their offsets, short
    filler lines between them. Every piece ends in '\\n' and so does the batch."""
    out = bytearray()
    for start, piece in sorted(placed):
        assert start >= len(out), (start, len(out))
        out += _fill(rng, start - len(out))
        out += piece
    assert len(out) <= total
    out += _fill(rng, total - len(out))
    assert len(out) == total and out[-1] == 0x0A
    return np.frombuffer(bytes(out), dtype=np.uint8)


def _straddler(rng, d, length, colon_at):
    """(start, line) of a line that starts d bytes before the boundary at 2 * TILE."""
    assert length > d
    return (2 * TILE - d, _line(rng, length, colon_at))


def _build_cases():
    rng = np.random.default_rng(0x0CC8)
    cases = {}
    # ---- halo: lines straddling a tile boundary that start d bytes before it --------------------
    for d in (511, 512, 513, 1447, 1448, 1535, 1536, 1537, 2047, 2048, 2049):
        if d < MAXL:   # valid, the colon before and after the boundary
            cases[f"halo_valid_{d}_colon_pre"] = _place(rng, 3 * TILE, [_straddler(rng, d, MAXL, d // 2)])
            cases[f"halo_valid_{d}_colon_post"] = _place(rng, 3 * TILE, [_straddler(rng, d, MAXL, min(d + (MAXL - d) // 2, MAXL - 2))])
            cases[f"halo_valid_{d}_shortest"] = _place(rng, 3 * TILE, [_straddler(rng, d, d + 1, d - 1)])
        too_long = max(MAXL + 1, d + 7)
        cases[f"halo_long_{d}"] = _place(rng, 3 * TILE, [_straddler(rng, d, too_long, d // 3)])
        cases[f"halo_long_{d}_nocolon"] = _place(rng, 3 * TILE, [_straddler(rng, d, too_long, None)])
    cases["halo_40000_byte_line"] = _place(rng, 4 * TILE, [(5000, _line(rng, 40000, 77))])
    cases["halo_40000_byte_line_from_0"] = _place(rng, 3 * TILE, [(0, _line(rng, 40000, 39990))])
    # a valid straddler whose only ':' is 1447 bytes before the boundary (its second byte)
    cases["halo_colon_1447_before"] = _place(rng, 3 * TILE, [_straddler(rng, 1448, MAXL, 1)])
    # straddlers into both later tiles of one batch, one found in the fast window, one in the halo
    cases["halo_two_boundaries"] = _place(rng, 3 * TILE, [(TILE - 300, _line(rng, 900, 10)),
                                                           (2 * TILE - 1440, _line(rng, MAXL, 1439))])
    # ---- 16-bit line ends and colons ------------------------------------------------------------
    for pos in (0, 1, TILE - 2, TILE - 1):
        end = TILE + pos   # '\n' at tile position pos of the second tile
        for tag, colon in (("colon", 2), ("nocolon", None)):
            cases[f"end_at_{pos}_{tag}"] = _place(rng, 3 * TILE, [(end - 39, _line(rng, 40, colon))])
    # ':' at tile position 16383, its '\n' in the next tile (first colon, and a second one after it)
    cases["colon_at_16383"] = _place(rng, 3 * TILE, [(2 * TILE - 21, _line(rng, 60, 20))])
    ln = bytearray(_line(rng, 60, 20))
    ln[30] = ord(":")
    cases["colon_at_16383_and_later"] = _place(rng, 3 * TILE, [(2 * TILE - 21, bytes(ln))])
    cases["colon_at_0_of_next_tile"] = _place(rng, 3 * TILE, [(2 * TILE - 21, _line(rng, 60, 21))])
    # more than 256 lines per tile, crossing window ends: 6-byte lines, runs of bare '\n'
    cases["six_byte_lines"] = np.frombuffer((b"a:1|c\n" * (2 * TILE // 6 + 1))[: 2 * TILE - 1] + b"\n", dtype=np.uint8)
    cases["six_byte_lines_high_bytes"] = np.frombuffer(
        (b"\xe9:1|c\n\x80\xff:7\n" * (3 * TILE // 11 + 1))[: 3 * TILE - 1] + b"\n", dtype=np.uint8)
    cases["bare_newlines"] = _place(rng, 3 * TILE, [(200, b"\n" * 1000), (TILE - 300, b"\n" * 700),
                                                    (2 * TILE - 1, b"\n\n"), (2 * TILE + 255, b"\n" * 258)])
    cases["all_newlines"] = np.full(2 * TILE, 0x0A, dtype=np.uint8)
    # ---- power tables: names over 64 bytes, straddling a boundary in their second / last segment -
    for n in (63, 64, 65, 127, 128, 129, 1023, 1447):
        nseg = (n + 63) // 64
        tail = b":1|c\n" if n + 5 <= MAXL else b":\n"
        last0 = (nseg - 1) * 64
        cuts = {"second": min(64 + 17, n - 1), "last": min(last0 + max((n - last0) // 2, 1), n - 1)}
        for tag, cut in cuts.items():   # `cut` name bytes lie before the boundary
            cases[f"name_{n}_{tag}_segment"] = _place(rng, 3 * TILE, [(2 * TILE - cut, _name(rng, n) + tail)])
        # and inside one tile, at every alignment of its start within a dword
        cases[f"name_{n}_inside"] = _place(rng, 2 * TILE, [(TILE + 3000 + k * 2000 + k, _name(rng, n) + tail)
                                                           for k in range(4)])
    return cases


@pytest.fixture(scope="module")
def cases():
    return _build_cases()


@pytest.fixture(scope="module")
def expected(cases, oracle):
    """The oracle's (records, hashes, count) per case and shard count, computed once."""
    return {(k, n): oracle.route(v, n) for k, v in cases.items() for n in SHARDS}


def _same(got, exp, what):
    (gr, gh, gn), (cr, ch, cn) = got, exp
    assert gn == cn, f"{what}: line count {gn} != {cn}"
    assert np.array_equal(gr, cr), f"{what}: records differ, first at {int(np.nonzero(gr != cr)[0][0])}"
    assert np.array_equal(gh, ch), f"{what}: hashes differ, first at {int(np.nonzero(gh != ch)[0][0])}"


def test_cases_are_what_they_claim(cases):
    """The builders themselves: sizes of two to four tiles, every batch ends in '\\n'."""
    assert len(cases) >= 80
    for k, v in cases.items():
        assert v.size in (2 * TILE, 3 * TILE, 4 * TILE) and v[-1] == 0x0A, k
    b = cases["halo_valid_1448_shortest"].tobytes()
    assert b[2 * TILE] == 0x0A and b[2 * TILE - 1449] == 0x0A and b.count(b"\n", 2 * TILE - 1448, 2 * TILE) == 0
    b = cases["colon_at_16383"].tobytes()
    assert b[2 * TILE - 1] == ord(":")


@pytest.mark.parametrize("n", SHARDS)
def test_each_case_alone(pkg, cases, expected, n):
    """One batch per launch (fewer than 8 batches: tiles dealt round-robin)."""
    with pkg.Router(n, 4 * TILE) as r:
        r.set_layout(pkg.SR_LAYOUT_UNIFORM)
        for k, v in cases.items():
            _same(r.route(v, want_hashes=True), expected[(k, n)], f"N={n} {k}")
            assert r.last_layout() == pkg.SR_LAYOUT_UNIFORM


class _Many:
    """Device buffers and descriptors of one route_device_many launch over `parts`."""

    def __init__(self, pkg, parts):
        import torch

        self.pkg, self.parts = pkg, parts
        caps = [max(int(p.size), 1) for p in parts]
        self.d_in = [torch.from_numpy(p.copy() if p.size else np.zeros(1, np.uint8)).to("cuda") for p in parts]
        self.d_out = [torch.empty(c * 8, dtype=torch.uint8, device="cuda") for c in caps]
        self.d_h = [torch.empty(c, dtype=torch.int64, device="cuda") for c in caps]
        self.d_n = torch.full((len(parts),), -1, dtype=torch.int64, device="cuda")
        self.descs = [(self.d_in[i].data_ptr(), int(p.size), self.d_out[i].data_ptr(), caps[i], self.d_h[i].data_ptr(),
                       self.d_n.data_ptr() + 8 * i) for i, p in enumerate(parts)]

    def clear(self):
        for t in self.d_out + self.d_h:
            t.zero_()
        self.d_n.fill_(-1)

    def check(self, exp, what):
        import torch

        torch.cuda.synchronize()
        counts = self.d_n.cpu().numpy()
        for i in range(len(self.parts)):
            k = int(counts[i])
            recs = self.d_out[i].cpu().numpy().view(self.pkg.RECORD_DTYPE)[:k]
            hs = self.d_h[i].cpu().numpy().view(np.uint64)[:k]
            _same((recs, hs, k), exp[i], f"{what}: batch {i}")


@pytest.mark.parametrize("n", SHARDS)
def test_cases_32_per_launch(pkg, cases, expected, n, torch_stream):
    """The same batches 32 to a launch (8+ batches: every batch within one XCD class)."""
    keys = sorted(cases)
    with pkg.Router(n, 4 * TILE) as r:
        r.set_layout(pkg.SR_LAYOUT_UNIFORM)
        r.set_stream(torch_stream.cuda_stream)
        for i0 in range(0, len(keys), 32):
            ks = keys[i0:i0 + 32]
            m = _Many(pkg, [cases[k] for k in ks])
            r.route_device_many(m.descs)
            m.check([expected[(k, n)] for k in ks], f"N={n} launch of {ks[0]}..")


def _shape_parts(cases, nb):
    """nb batches of 0 B, 1 B and one to three tiles (whole and partial last tiles)."""
    keys = sorted(cases)
    parts = []
    for i in range(nb):
        src = cases[keys[(7 * i) % len(keys)]]
        if i % 8 == 3:
            parts.append(np.frombuffer(b"", dtype=np.uint8))
        elif i % 8 == 5:
            parts.append(np.frombuffer(b"\n", dtype=np.uint8))
        else:
            cut = [TILE, 2 * TILE, 3 * TILE, TILE + 1, 3 * TILE - 777][i % 5]
            p = src[:cut].copy()
            p[-1] = 0x0A
            parts.append(p)
    return parts


@pytest.mark.parametrize("n,nb", [(4, 9), (16, 9), (4, 32), (16, 32)])
def test_launch_shapes_and_graph_replay(pkg, oracle, cases, n, nb, torch_stream):
    """9 batches (the smallest XCD-class launch) and 32 batches with empty, one-byte and one- to
    three-tile batches: three launches back to back on one context, then one replayed from a captured
    graph, each checked batch by batch."""
    import torch

    parts = _shape_parts(cases, nb)
    exp = [oracle.route(p, n) for p in parts]
    with pkg.Router(n, 4 * TILE) as r:
        r.set_layout(pkg.SR_LAYOUT_UNIFORM)
        r.set_stream(torch_stream.cuda_stream)
        m = _Many(pkg, parts)
        for _ in range(3):
            r.route_device_many(m.descs)
        m.check(exp, f"N={n}, {nb} batches, third launch")
        assert r.last_layout() == pkg.SR_LAYOUT_UNIFORM
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch_stream):
            r.route_device_many(m.descs)
        m.clear()
        g.replay()
        m.check(exp, f"N={n}, {nb} batches, graph replay")
        m.clear()
        g.replay()
        g.replay()
        m.check(exp, f"N={n}, {nb} batches, replayed twice more")
