"""Every route kernel variant on hostile bytes: the byte-exact batches of test_gpu_route_occupancy.py
(halo, 16-bit positions, power tables) and the signed names of byte_streams.extreme_name_cases(), 32 to
a launch, under each forced lane layout and each shard state below; records, hashes, counts and
probed-dead bitmaps against the CPU oracle, bit for bit, the outputs prefilled with a sentinel.

The shard states and the branch of launch_route (route_host.hpp) each one takes:

| N, dead | path exercised |
|---|---|
| 4, 0 and 16, 0 | KV_ALIVE (uniform, segments and chunks) |
| 7, 1 (dead first) and 64, 1 (dead last) | KV_DEAD1 |
| 5, 2 and 64, 4 | KV_DEFER1, probe_defer_kernel<4> |
| 64, 8 and 64, 16 | probe_defer_kernel<8>, <16> |
| 100, 3 and 100, 16 | N > 64: the picks variant with LDS pads |
| 64, 17 and 1000, 600 | wide probe, one launch per batch |
| 1100, 2 | bitmap by probed_dead_kernel replay (N > 1024) |
| 3, 3 | every shard dead |

Dead shards are a seeded sample except where first or last is stated. Route + pack over the signed
names runs KV_DEAD1 | KV_HIST1 (7, 1) and the all-alive histograms (4, 0). Captured launches with dead
shards: without hash arrays and before anything else ran on the context a launch with two or more dead
shards cannot defer its probes (the context's scratch holds max_batch_bytes / 6 + 1 hashes, the
launch's batches need one per record slot), and runs the full-probe kernel. A batch at base offsets
0..15 between poison must route as the same bytes do alone. Needs an MI355X: `pytest -m gpu`."""
from __future__ import annotations

import random

import numpy as np
import pytest

import byte_streams as B
from test_gpu_mtu import _check_pack
from test_gpu_route_occupancy import _build_cases

pytestmark = pytest.mark.gpu

TILE = B.TILE
SENTINEL = 0x5A5A5A5A5A5A5A5A
SLACK = 64                      # record slots past a batch's line count, which must keep the sentinel
PER_LAUNCH = 32

# (N, dead, which): which = "first" / "last" / "sample"
STATES = [(4, 0, "sample"), (16, 0, "sample"), (7, 1, "first"), (64, 1, "last"), (5, 2, "sample"), (64, 4, "sample"),
          (64, 8, "sample"), (64, 16, "sample"), (100, 3, "sample"), (100, 16, "sample"), (64, 17, "sample"),
          (1000, 600, "sample"), (1100, 2, "sample"), (3, 3, "sample")]
LAYOUTS = ["UNIFORM", "SEGMENTS", "CHUNKS"]


def _alive(n, dead, which="sample"):
    alive = [1] * n
    if which == "first":
        ks = range(dead)
    elif which == "last":
        ks = range(n - dead, n)
    else:
        ks = random.Random(1000 * n + dead).sample(range(n), dead)
    for k in ks:
        alive[k] = 0
    return alive


def _state_id(s):
    return f"N{s[0]}_dead{s[1]}" + ("" if s[2] == "sample" else f"_{s[2]}")


@pytest.fixture(scope="module")
def cases():
    c = dict(_build_cases())
    extreme = B.extreme_name_cases()
    assert not set(c) & set(extreme)
    c.update(extreme)
    return c


@pytest.fixture(scope="module")
def dev_cases(cases):
    """Every case's bytes on the device, uploaded once."""
    import torch

    return {k: torch.from_numpy(v.copy()).to("cuda") for k, v in cases.items()}


@pytest.fixture(scope="module")
def expected(cases, oracle):
    """(N, dead, which) -> {case: (records, hashes, count, probed-dead shard ids)} from the oracle; the
    last state asked for is kept (the layouts of one state run back to back)."""
    memo = {}

    def get(state):
        if state not in memo:
            memo.clear()
            n, dead, which = state
            alive = _alive(n, dead, which)
            memo[state] = {k: oracle.route(v, n, alive) + (oracle.probed_dead(v, n, alive).tolist(),)
                           for k, v in cases.items()}
        return memo[state]

    return get


class _Launch:
    """Device outputs and descriptors of one route_device_many launch: record slots, hash slots, counts
    and bitmaps all prefilled with SENTINEL. caps: record slots per batch."""

    def __init__(self, pkg, n_shards, d_ins, sizes, caps, hashes=True, bitmaps=True):
        import torch

        self.pkg, self.n_shards, self.caps, self.nw = pkg, n_shards, caps, max((n_shards + 63) // 64, 1)
        nb, width = len(d_ins), max(caps)
        self.d_out = torch.empty((nb, width), dtype=torch.int64, device="cuda")
        self.d_h = torch.empty((nb, width), dtype=torch.int64, device="cuda") if hashes else None
        self.d_n = torch.empty(nb, dtype=torch.int64, device="cuda")
        self.d_pd = torch.empty((nb, self.nw), dtype=torch.int64, device="cuda") if bitmaps else None
        self.clear()
        self.descs = [(d_ins[i].data_ptr() if not isinstance(d_ins[i], int) else d_ins[i], int(sizes[i]),
                       self.d_out[i].data_ptr(), int(caps[i]), self.d_h[i].data_ptr() if hashes else None,
                       self.d_n[i].data_ptr(), self.d_pd[i].data_ptr() if bitmaps else None) for i in range(nb)]

    def clear(self):
        for t in (self.d_out, self.d_h, self.d_n, self.d_pd):
            if t is not None:
                t.fill_(SENTINEL)

    def check(self, exp, what):
        """exp: per batch (records, hashes, count, probed shard ids) of the oracle."""
        import torch

        torch.cuda.synchronize()
        out = self.d_out.cpu().numpy()
        hs = self.d_h.cpu().numpy().view(np.uint64) if self.d_h is not None else None
        counts = self.d_n.cpu().numpy()
        pd = self.d_pd.cpu().numpy().view(np.uint64) if self.d_pd is not None else None
        for i, (er, eh, en, ep) in enumerate(exp):
            w = f"{what}: batch {i}"
            cap = self.caps[i]
            k = min(en, cap)
            assert int(counts[i]) == en, f"{w}: line count {int(counts[i])} != {en}"
            got = out[i, :k].view(self.pkg.RECORD_DTYPE)
            assert np.array_equal(got, er[:k]), f"{w}: records differ, first at {int(np.nonzero(got != er[:k])[0][0])}"
            assert (out[i, k:cap] == SENTINEL).all(), f"{w}: a record slot past the count was written"
            if hs is not None:
                assert np.array_equal(hs[i, :k], eh[:k]), f"{w}: hashes differ, first at {int(np.nonzero(hs[i, :k] != eh[:k])[0][0])}"
                assert (hs[i, k:cap] == np.uint64(SENTINEL)).all(), f"{w}: a hash slot past the count was written"
            if pd is not None:
                assert self.pkg.bitmap_shards(pd[i], self.n_shards).tolist() == ep, f"{w}: probed-dead bitmap"
                assert int(pd[i, -1]) >> (((self.n_shards - 1) & 63) + 1) == 0, f"{w}: bitmap bits past N"


def test_cases_cover_both_sources(cases):
    assert len(cases) >= 300 and all(v[-1] == 0x0A and v.size in (2 * TILE, 3 * TILE, 4 * TILE) for v in cases.values())
    assert "halo_valid_1448_shortest" in cases and "uniform_1447_straddle_1446" in cases


@pytest.mark.parametrize("layout", LAYOUTS)     # the upper decorator varies fastest: a state's layouts run back to back
@pytest.mark.parametrize("state", STATES, ids=_state_id)
def test_variants_32_per_launch(pkg, cases, dev_cases, expected, torch_stream, state, layout):
    """Every case, 32 batches to a route_device_many launch with hashes and probed-dead bitmaps."""
    n, dead, which = state
    lay = getattr(pkg, "SR_LAYOUT_" + layout)
    exp = expected(state)
    keys = sorted(cases)
    with pkg.Router(n, 4 * TILE) as r:
        r.set_layout(lay)
        r.set_alive(_alive(n, dead, which))
        r.set_stream(torch_stream.cuda_stream)
        for i0 in range(0, len(keys), PER_LAUNCH):
            ks = keys[i0:i0 + PER_LAUNCH]
            m = _Launch(pkg, n, [dev_cases[k] for k in ks], [cases[k].size for k in ks],
                        [exp[k][2] + SLACK for k in ks])
            r.route_device_many(m.descs)
            assert r.last_layout() == lay
            m.check([exp[k] for k in ks], f"{layout} {_state_id(state)} launch of {ks[0]}..")


@pytest.mark.parametrize("n,dead,which", [(7, 1, "first"), (4, 0, "sample")])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_route_pack_signed_names(pkg, oracle, n, dead, which, layout):
    """Route + pack (one dead: KV_DEAD1 | KV_HIST1; all alive: the tile histograms) over every signed
    name in one batch, against the oracle's packing."""
    data = np.concatenate(list(B.extreme_name_cases().values()))
    alive = _alive(n, dead, which)
    rng = np.random.default_rng(n)
    with pkg.Router(n, int(data.size)) as r:
        r.set_layout(getattr(pkg, "SR_LAYOUT_" + layout))
        r.set_alive(alive)
        for fill in (None, rng.integers(0, 1451, n).tolist()):
            _check_pack(pkg, oracle, data, n, alive, fill, r)
        assert r.last_layout() == getattr(pkg, "SR_LAYOUT_" + layout)


CAPTURE_CASES = ["uniform_1447_straddle_64", "x80_1025_straddle_17", "xff_257_inside", "alt_129_inside",
                 "uniform_1023_straddle_1022", "halo_valid_1448_colon_post", "name_1447_last_segment",
                 "six_byte_lines_high_bytes", "colon_at_16383"]


@pytest.mark.parametrize("n,dead,which", [(5, 2, "sample"), (64, 16, "sample"), (64, 17, "sample"), (7, 1, "first")])
@pytest.mark.parametrize("mode", ["no_hashes", "hashes"])
@pytest.mark.parametrize("layout", ["AUTO"] + LAYOUTS)
def test_captured_launches_with_dead_shards(pkg, oracle, cases, dev_cases, torch_stream, n, dead, which, mode, layout):
    """One route_device_many of 9 batches captured into a graph on a fresh context, replayed three
    times. no_hashes: nothing ran on the context before the capture and no batch has a hash array, so
    with two or more dead shards the launch cannot defer (asserted from the inputs below) and runs the
    full-probe kernel; hashes: the deferral into the batches' hash arrays is captured."""
    import torch

    max_batch = 4 * TILE
    alive = _alive(n, dead, which)
    parts = [cases[k] for k in CAPTURE_CASES]
    exp = [oracle.route(p, n, alive) + (oracle.probed_dead(p, n, alive).tolist(),) for p in parts]
    caps = [int(p.size) for p in parts]
    if mode == "no_hashes":   # the deferral's scratch (sized by sr_set_alive) cannot hold the launch, or even one batch
        assert sum(caps) > min(caps) > max_batch // 6 + 1
    with pkg.Router(n, max_batch) as r:
        r.set_layout(getattr(pkg, "SR_LAYOUT_" + layout))
        r.set_alive(alive)
        r.set_stream(torch_stream.cuda_stream)
        m = _Launch(pkg, n, [dev_cases[k] for k in CAPTURE_CASES], caps, caps, hashes=mode == "hashes")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch_stream):
            r.route_device_many(m.descs)
        m.clear()
        g.replay()
        m.check(exp, f"{layout} N={n} dead={dead} {mode}: first replay")
        m.clear()
        g.replay()
        g.replay()
        m.check(exp, f"{layout} N={n} dead={dead} {mode}: replayed twice more")
        # the same context outside capture afterwards
        m.clear()
        r.route_device_many(m.descs)
        m.check(exp, f"{layout} N={n} dead={dead} {mode}: plain launch after the graph")


ALIGN_RESIDUES = (0, 1, 5, 15)
ALIGN_LEADS = (0, 1, 2, 3, 4, 7, 8, 13, 15)


@pytest.fixture(scope="module")
def aligned_inputs():
    """Per nbytes residue: the 3-tile prefix of the ragged stream cut at a '\\n', and per lead its copy
    between '\\n:' poison on the device."""
    import torch

    stream = B.ragged_stream(1, B.RAGGED_MIN_BYTES)
    out = {}
    for res in ALIGN_RESIDUES:
        batch = B.cut_at_newline(stream, 2 * TILE, 3 * TILE, res)
        assert batch.size % 16 == res and 2 * TILE < batch.size <= 3 * TILE
        placed = []
        for lead in ALIGN_LEADS:
            buf, off = B.embed(batch, lead, b"\n:")
            t = torch.from_numpy(buf.copy()).to("cuda")
            assert (t.data_ptr() + off) % 16 == lead
            placed.append((lead, t, off))
        out[res] = (batch, placed)
    return out


@pytest.mark.parametrize("n,dead,which", [(16, 0, "sample"), (7, 1, "first")])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_unaligned_base_and_poison(pkg, oracle, aligned_inputs, torch_stream, n, dead, which, layout):
    """sr_route.h asks no alignment of d_bytes and no padding: a batch at base offsets 0..15 (mod 16),
    sizes = 0, 1, 5, 15 (mod 16), '\\n:' poison right before and after it, routes as the oracle routes
    the batch alone (a poison byte read as data moves a line end or a first colon)."""
    alive = _alive(n, dead, which)
    lay = getattr(pkg, "SR_LAYOUT_" + layout)
    with pkg.Router(n, 4 * TILE) as r:
        r.set_layout(lay)
        r.set_alive(alive)
        r.set_stream(torch_stream.cuda_stream)
        for res, (batch, placed) in aligned_inputs.items():
            e = oracle.route(batch, n, alive) + (oracle.probed_dead(batch, n, alive).tolist(),)
            m = _Launch(pkg, n, [t.data_ptr() + off for _, t, off in placed], [batch.size] * len(placed),
                        [e[2] + SLACK] * len(placed))
            for d in m.descs:   # one batch per launch: its tiles start at its own base
                r.route_device_many([d])
            assert r.last_layout() == lay
            m.check([e] * len(placed), f"{layout} N={n} dead={dead} size%16={res} leads {ALIGN_LEADS}")
            m.clear()
            r.route_device_many(m.descs)   # and the nine placements in one launch
            m.check([e] * len(placed), f"{layout} N={n} dead={dead} size%16={res} one launch")
