"""CPU: the builders of tests/density_streams.py are what they claim, measured with the oracle's own line
split and verdicts. These are conditions on the inputs of tests/test_gpu_route_density.py, which
therefore never skips or filters a case.

What a wave of the route kernel's uniform layout hashes is restated here from the oracle's records: a
tile's lines are those whose '\\n' lies in it, hashed in rounds of 256 lines; with G lanes per line
(density_streams.expected_G of the tile's '\\n' count) line jj of a round sits on the flattened lanes
jj G .. jj G + G - 1, a wave is 64 consecutive flattened lanes, a valid line's name [s, c) has
max((E - s + 63) >> 6, 0) windows with E = c rounded up to 16, an invalid line has none, and lane gi of a
line runs ceil((windows - gi) / G) trips of the window loop, clipped at 0."""
from __future__ import annotations

import numpy as np
import pytest

import byte_streams as B
import density_streams as D

TILE, NL, COLON = B.TILE, B.NL, B.COLON
INVALID_FROM = 0xFFFD          # SR_ROUTE_INVALID_LENGTH: the smallest route code that is no shard


@pytest.fixture(scope="module")
def batches():
    return D.all_batches()


class _Lines:
    """Every line of a batch, from the oracle's records (none dropped: asserted against the '\\n' bytes)."""

    def __init__(self, data, oracle):
        recs, _, n = oracle.route(data, 4)
        ends = np.flatnonzero(data == NL)
        assert n == len(recs) == ends.size and data[-1] == NL
        self.n, self.data, self.end = n, data, ends
        self.start = np.concatenate([[0], ends[:-1] + 1])
        assert np.array_equal(recs["offset"].astype(np.int64), self.start)
        assert np.array_equal(recs["length"].astype(np.int64), ends - self.start + 1)   # no line of 65535 bytes or more
        self.valid = recs["route"] < INVALID_FROM
        colons = np.flatnonzero(data == COLON)
        idx = np.searchsorted(colons, self.start)
        col = colons[np.minimum(idx, colons.size - 1)]
        has = (idx < colons.size) & (col < ends)
        length = ends - self.start + 1
        assert np.array_equal(self.valid, has & (length >= 6) & (length <= B.MAXL))
        self.colon = np.where(self.valid, col, -1)
        self.nlen = np.where(self.valid, self.colon - self.start, -1)       # name bytes; -1: invalid line
        E = (self.colon + 15) & ~15
        self.windows = np.where(self.valid, np.maximum((E - self.start + 63) >> 6, 0), 0)
        self.tile = ends // TILE
        self.counts = np.bincount(self.tile)
        self.jj = np.arange(n) - np.searchsorted(self.tile, self.tile)      # index among its tile's lines
        self.G = np.array([D.expected_G(int(c)) if c else 0 for c in self.counts])[self.tile]

    def name(self, i):
        return self.data[self.start[i]: self.colon[i]].tobytes()

    def waves(self):
        """(G, line indices) of every wave of every round of every tile."""
        for t, count in enumerate(self.counts.tolist()):
            if not count:
                continue
            G, first = D.expected_G(count), int(np.searchsorted(self.tile, t))
            for w0 in range(0, count, D.WIN):
                nwin = min(D.WIN, count - w0)
                for x0 in range(0, nwin * G, 64):
                    j0, j1 = x0 // G, min((x0 + 63) // G + 1, nwin)
                    yield G, np.arange(first + w0 + j0, first + w0 + j1)

    def trips(self, i, G):
        """Per-lane trip counts of line i on G lanes."""
        return [max(-(-(int(self.windows[i]) - gi) // G), 0) for gi in range(G)]


@pytest.fixture(scope="module")
def lines(batches, oracle):
    return {k: _Lines(v, oracle) for k, v in batches.items()}


def test_seeded_sized_and_ending_in_newline(batches):
    assert list(batches) == [f"G{G}" for G in D.GROUPS] + ["threshold"]
    again = D.all_batches()
    for k, v in batches.items():
        assert v.dtype == np.uint8 and v[-1] == NL and np.array_equal(v, again[k]), k
        assert v.size % 16 == D.TAIL_RESIDUE and 0 < v.size % TILE < 200, k
        assert v.size <= 64 * TILE + 200, (k, v.size // TILE)
    assert sum(v.size for v in batches.values()) + batches["G4"].size < 8 << 20


def test_expected_G_is_the_table():
    table = {1: 32, 15: 32, 16: 16, 31: 16, 32: 8, 63: 8, 64: 4, 127: 4, 128: 2, 252: 2, 253: 1, 256: 1, 257: 1,
             16384: 1}
    assert {c: D.expected_G(c) for c in table} == table
    for G, (lo, hi) in D.COUNT_RANGE.items():
        assert all(D.expected_G(c) == G for c in (lo, hi)) and all(lo <= c <= hi for c in D.TILE_COUNTS[G])
        assert lo in (D.TILE_COUNTS[G] + (lo,)) and (hi in D.TILE_COUNTS[G] or G == 1)
        assert G == 32 or D.expected_G(lo - 1) == 2 * G


@pytest.mark.parametrize("G", D.GROUPS)
def test_tile_counts_lie_in_the_class(lines, G):
    ln = lines[f"G{G}"]
    lo, hi = D.COUNT_RANGE[G]
    full = ln.counts[:-1]
    assert ln.counts.size == ln.data.size // TILE + 1 and full.size >= 8
    assert ((full >= lo) & (full <= hi)).all(), full.tolist()
    assert all(D.expected_G(int(c)) == G for c in full)
    assert lo in full.tolist() and (G == 1 or hi in full.tolist())
    if G == 1:   # both sides of the 256-line round
        assert {253, 256, 257} <= set(full.tolist()) and full.max() >= 512
    # the partial tile holds valid lines only
    last = ln.tile == ln.counts.size - 1
    assert last.sum() >= 2 and ln.valid[last].all()


def test_threshold_tile_counts_are_exact(lines):
    ln = lines["threshold"]
    assert tuple(ln.counts[:-1].tolist()) == D.THRESHOLD_COUNTS
    assert [D.expected_G(c) for c in D.THRESHOLD_COUNTS] == [32, 16, 16, 8, 8, 4, 4, 2, 2, 1, 1, 1]
    for t in range(len(D.THRESHOLD_COUNTS)):
        sel = np.flatnonzero((ln.tile == t) & ln.valid & (ln.nlen >= 129) & (ln.start % 16 != 0) & (ln.start // TILE == t))
        assert any(max(ln.name(i)) >= 0x80 for i in sel), t
    assert ln.valid[ln.tile == len(D.THRESHOLD_COUNTS)].all()


@pytest.mark.parametrize("G", D.GROUPS)
def test_alignment_grid_lengths_and_classes(lines, G):
    ln = lines[f"G{G}"]
    v = np.flatnonzero(ln.valid)
    pairs = set(zip((ln.start[v] % 16).tolist(), (ln.colon[v] % 16).tolist()))
    assert len(pairs) == 256, sorted({(a, b) for a in range(16) for b in range(16)} - pairs)
    # every length class, within +-15
    want = D.edge_lengths(G)
    assert {0, 1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1443, 1447} <= set(want)
    assert {n for n in (64 * G - 1, 64 * G, 64 * G + 1, 128 * G + 1) if n <= D.MAX_NAME} <= set(want)
    nl = ln.nlen[v]
    for n in want:
        assert (np.abs(nl - n) <= 15).any(), n
    assert nl.max() == D.MAX_NAME and nl.min() == 0
    # every name class at one window, two windows and the most there are
    top = int(ln.windows.max())
    assert top == 23
    seen = {}
    for i in v:
        name = ln.name(i)
        if not name:
            continue
        a = np.frombuffer(name, dtype=np.uint8)
        w = int(ln.windows[i])
        for cls, ok in (("x80", (a == 0x80).all()), ("xff", (a == 0xFF).all()), ("x7f", (a == 0x7F).all()),
                        ("alt", a.size > 1 and (a[0::2] == 0x80).all() and (a[1::2] == 0x7F).all()),
                        ("uniform", a.size > 3 and np.unique(a).size > 2)):
            if ok:
                seen.setdefault(w, set()).add(cls)
    for w in (1, 2, top):
        assert seen[w] == set(B.NAME_CLASSES), (w, seen[w])


@pytest.mark.parametrize("G", D.GROUPS)
def test_waves_mix_trip_counts(lines, G):
    ln = lines[f"G{G}"]
    top = max(max(ln.trips(i, g)) for g, idx in ln.waves() for i in idx)
    assert top == -(-23 // G)
    longest, short_only, zeros, valid_empty, no_colon = [], [], [], [], []
    for g, idx in ln.waves():
        assert g == G or idx[0] >= ln.n - 8      # (the partial tile's few lines get 32 lanes each)
        one_piece = [i for i in idx if ln.nlen[i] >= 1 and ln.start[i] >> 4 == (ln.colon[i] - 1) >> 4]
        # (32 lanes per line: every name takes one trip, so the name of the most windows, 23 busy lanes)
        most = [i for i in idx if max(ln.trips(i, g)) == top and (G < 32 or ln.windows[i] == 23)]
        if any(i != j for i in most for j in one_piece):
            longest.append(idx[0])
        if len(idx) == 64 // g and ln.valid[idx].all() and (ln.nlen[idx] <= 16).all() and (ln.nlen[idx] >= 1).all():
            short_only.append(idx[0])
        multi = [i for i in idx if ln.windows[i] >= 2]
        invalid = [i for i in idx if not ln.valid[i]]
        empty = [i for i in idx if ln.data[ln.start[i]] == COLON]
        if multi and G < 32 and any(i != j for i in invalid for j in empty):
            zeros.append(idx[0])
        if multi and G == 32 and any(i in invalid for i in empty):     # ':1|c' is both
            zeros.append(idx[0])
        if multi and any(ln.valid[i] for i in empty):
            valid_empty.append(idx[0])
        if multi and any(ln.colon[i] < 0 and ln.end[i] - ln.start[i] >= 6 for i in invalid):
            no_colon.append(idx[0])
    for what, found in (("longest beside one piece", longest), ("short names only", short_only),
                        ("multi-window beside invalid and empty", zeros), ("beside a valid empty name", valid_empty),
                        ("beside a line without a colon", no_colon)):
        assert len(found) >= 2, (what, found)
    # a long name among short ones: lanes of one wave that differ by the whole range of trip counts
    spread = max(max(max(ln.trips(i, g)) for i in idx) - min(min(ln.trips(i, g)) for i in idx) for g, idx in ln.waves())
    assert spread == top


@pytest.mark.parametrize("G", D.GROUPS)
def test_neighbours_bytes_share_a_piece(lines, G):
    ln = lines[f"G{G}"]
    d = ln.data
    v = np.flatnonzero(ln.valid & (ln.nlen >= 1) & (ln.start >= 2))
    # a name that starts mid-piece, the previous line's last byte before its '\n' >= 0x80 in the same piece
    after = v[(ln.start[v] % 16 >= 2) & (d[ln.start[v] - 2] >= 0x80)]
    # a name whose ':' is followed by a byte >= 0x80 in the same piece
    before = v[(ln.colon[v] % 16 <= 14) & (d[ln.colon[v] + 1] >= 0x80)]
    for sel in (after, before):
        assert sel.size >= 16 and (ln.windows[sel] >= 2).any() and (ln.windows[sel] == 1).any()


def _straddlers(ln):
    """Per tile boundary with one, the valid line of two or more windows that starts before and ends after."""
    out = {}
    for i in np.flatnonzero(ln.valid & (ln.start // TILE < ln.end // TILE) & (ln.windows >= 2)):
        out[int(ln.end[i] // TILE) * TILE] = i
    return out


@pytest.mark.parametrize("G", D.GROUPS)
def test_straddlers_sit_where_asked(lines, G):
    ln = lines[f"G{G}"]
    found = _straddlers(ln)
    assert len(found) >= 4
    rel = {(int(ln.start[i]) - b, int(ln.colon[i]) - b) for b, i in found.items()}
    assert any(s == -1448 for s, _ in rel), "none starts 1448 bytes before its boundary"
    assert any(c == -1 for _, c in rel) and any(c == 0 for _, c in rel), "':' on the last byte before / the first after"
    assert sum(s < 0 < c for s, c in rel) >= 2, "names lying partly before the boundary"
    assert rel == {(-d, n - d) for d, n, _, _ in D.STRADDLERS}
    # every line that crosses a boundary is one of them or an invalid one
    cross = np.flatnonzero(ln.start // TILE < ln.end // TILE)
    assert all((not ln.valid[i]) or i in found.values() for i in cross)


def test_threshold_straddlers(lines):
    ln = lines["threshold"]
    rel = {(b // TILE, int(ln.start[i]) - b, int(ln.colon[i]) - b) for b, i in _straddlers(ln).items()}
    assert rel == {(4, -70, 130), (9, -151, -1)}
