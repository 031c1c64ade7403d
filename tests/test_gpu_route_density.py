"""The name hash at every lanes-per-line group size G: the batches of tests/density_streams.py (one per
G in 1, 2, 4, 8, 16, 32, built tile by tile so that the kernel picks that G, and one whose tiles sit on
the '\\n' counts where G flips) against the CPU oracle, records, hashes, line counts and probed-dead
bitmaps bit for bit, the outputs prefilled with a sentinel. tests/test_density_streams.py shows on the CPU
what the batches hold.

| launch | kernel path |
|---|---|
| UNIFORM, N = 4 and 16, all alive | the KV_UNIFORM, KV_ALIVE route_kernel: sdbm_mx, the matrix-core hash over G lanes |
| SEGMENTS and CHUNKS, N = 4, all alive | the segment layout's VALU hash, route_chunk_kernel |
| UNIFORM, N = 7 with the first dead, N = 5 with two dead | KV_DEAD1 and KV_DEFER1: sdbm_img over the same G lanes |
| one route_device_many of eight batches, plain and replayed from a graph | one XCD class per batch |
| each density batch at base offset 5 between bytes >= 0x80 | the image load at an unaligned base |

Needs an MI355X: `pytest -m gpu`."""
from __future__ import annotations

import pytest

import byte_streams as B
import density_streams as D
from test_gpu_route_variants import SLACK, _alive, _Launch

pytestmark = pytest.mark.gpu

NAMES = [f"G{G}" for G in D.GROUPS] + ["threshold"]
# (layout, N, dead, which) besides the all-alive uniform launches
VARIANTS = [("SEGMENTS", 4, 0, "sample"), ("CHUNKS", 4, 0, "sample"), ("UNIFORM", 7, 1, "first"), ("UNIFORM", 5, 2, "sample")]
POISON = b"\x80\xff\x8a\xba\xfe"     # '\n' and ':' with bit 7 set among them


@pytest.fixture(scope="module")
def batches():
    return D.all_batches()


@pytest.fixture(scope="module")
def dev(batches):
    """Every batch on the device, uploaded once."""
    import torch

    return {k: torch.from_numpy(v.copy()).to("cuda") for k, v in batches.items()}


@pytest.fixture(scope="module")
def expected(batches, oracle):
    """(batch, N, dead, which) -> (records, hashes, count, probed-dead shard ids) of the oracle, computed once."""
    memo = {}

    def get(name, n, dead=0, which="sample"):
        key = (name, n, dead, which)
        if key not in memo:
            alive = _alive(n, dead, which)
            v = batches[name]
            memo[key] = oracle.route(v, n, alive) + (oracle.probed_dead(v, n, alive).tolist(),)
        return memo[key]

    return get


def _one(pkg, r, n, d_in, size, exp, what):
    """One batch, one launch, checked."""
    m = _Launch(pkg, n, [d_in], [size], [exp[2] + SLACK])
    r.route_device_many(m.descs)
    m.check([exp], what)
    return m


@pytest.mark.parametrize("n", [4, 16])
@pytest.mark.parametrize("name", NAMES)
def test_uniform_all_alive(pkg, batches, dev, expected, torch_stream, name, n):
    """The matrix-core variant, each batch alone on a context of its own size."""
    size = int(batches[name].size)
    with pkg.Router(n, size) as r:
        r.set_layout(pkg.SR_LAYOUT_UNIFORM)
        r.set_stream(torch_stream.cuda_stream)
        _one(pkg, r, n, dev[name], size, expected(name, n), f"{name} N={n} uniform")
        assert r.last_layout() == pkg.SR_LAYOUT_UNIFORM


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"{v[0]}_N{v[1]}_dead{v[2]}")
@pytest.mark.parametrize("name", NAMES)
def test_other_variants(pkg, batches, dev, expected, torch_stream, name, variant):
    """The variants that keep the VALU hash (and the chunk kernel) on the same batches."""
    layout, n, dead, which = variant
    lay = getattr(pkg, "SR_LAYOUT_" + layout)
    size = int(batches[name].size)
    with pkg.Router(n, size) as r:
        r.set_layout(lay)
        r.set_alive(_alive(n, dead, which))
        r.set_stream(torch_stream.cuda_stream)
        _one(pkg, r, n, dev[name], size, expected(name, n, dead, which), f"{name} {layout} N={n} dead={dead}")
        assert r.last_layout() == lay


def test_eight_batches_one_launch(pkg, batches, dev, expected, torch_stream):
    """The seven batches and the G = 4 one again in one route_device_many (eight batches: each batch's
    tiles on one XCD class), plain, then captured into a graph and replayed once."""
    import torch

    n = 4
    names = NAMES + ["G4"]
    exp = [expected(k, n) for k in names]
    sizes = [int(batches[k].size) for k in names]
    with pkg.Router(n, max(sizes)) as r:
        r.set_layout(pkg.SR_LAYOUT_UNIFORM)
        r.set_stream(torch_stream.cuda_stream)
        m = _Launch(pkg, n, [dev[k] for k in names], sizes, [e[2] + SLACK for e in exp])
        r.route_device_many(m.descs)
        assert r.last_layout() == pkg.SR_LAYOUT_UNIFORM
        m.check(exp, "eight batches, plain launch")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch_stream):
            r.route_device_many(m.descs)
        m.clear()
        g.replay()
        m.check(exp, "eight batches, graph replay")


@pytest.mark.parametrize("G", D.GROUPS)
def test_base_offset_5_between_poison(pkg, batches, dev, expected, torch_stream, G):
    """A batch 5 bytes past a 16-byte boundary, bytes >= 0x80 right before and after it, routes as the
    same bytes do alone: as the oracle says, and as the device said for the aligned copy."""
    import torch

    n, name = 4, f"G{G}"
    batch = batches[name]
    buf, off = B.embed(batch, 5, POISON)
    assert min(POISON) >= 0x80 and buf[off - 1] >= 0x80 and buf[off + batch.size] >= 0x80
    t = torch.from_numpy(buf.copy()).to("cuda")
    assert (t.data_ptr() + off) % 16 == 5
    exp = expected(name, n)
    with pkg.Router(n, int(batch.size)) as r:
        r.set_layout(pkg.SR_LAYOUT_UNIFORM)
        r.set_stream(torch_stream.cuda_stream)
        alone = _one(pkg, r, n, dev[name], int(batch.size), exp, f"{name} alone")
        moved = _one(pkg, r, n, t.data_ptr() + off, int(batch.size), exp, f"{name} at base offset 5")
        assert r.last_layout() == pkg.SR_LAYOUT_UNIFORM
        assert torch.equal(alone.d_out, moved.d_out) and torch.equal(alone.d_h, moved.d_h)
        assert torch.equal(alone.d_n, moved.d_n) and torch.equal(alone.d_pd, moved.d_pd)
