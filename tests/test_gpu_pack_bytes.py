"""The owner pack (regroup_kernel.hpp) and the MTU packing on ragged bytes: byte_streams.ragged_stream
holds valid lines of every length 6..1449 at every (start, length) alignment mod 16, names of any byte
value, invalid lines of every kind, a run of 1449-byte lines that crosses several copy windows and a run
of invalid lines that leaves pack tiles empty (tests/test_byte_streams.py checks all that on the CPU).
Every output buffer is prefilled, and compared whole: the zero fill between lines and every byte past
the packed total count. Batches whose last line ends at the batch's last byte sit at odd base addresses
between 0xEE poison, which must not show up anywhere.

The pack's tile has two 256-record chunks unless the batches' bytes exceed 192 per record slot
(pack_chunks_for in sr_route.hip: `bytes > 192 * max_records` -> one chunk): max_records = nbytes takes
two chunks, max_records = the line count one (asserted from the inputs). Needs an MI355X: `pytest -m gpu`."""
from __future__ import annotations

import random

import numpy as np
import pytest

import byte_streams as B
from test_gpu_mtu import _check_pack

pytestmark = pytest.mark.gpu

RAGGED_BYTES = 3 << 20
PACK_CHUNK_BYTES_PER_SLOT = 192   # pack_chunks_for: one chunk per tile above this many bytes per record slot


def _alive(n, dead):
    alive = [1] * n
    for k in random.Random(77 * n + dead).sample(range(n), dead):
        alive[k] = 0
    return alive


def _chunks(total_bytes, total_slots):
    """pack_chunks_for restated from the inputs."""
    return 1 if total_bytes > PACK_CHUNK_BYTES_PER_SLOT * max(total_slots, 1) else 2


@pytest.fixture(scope="module")
def ragged():
    return B.ragged_stream(1, RAGGED_BYTES)


@pytest.fixture(scope="module")
def routed(ragged, oracle):
    """(n_shards, dead) -> (alive, the oracle's records of the whole stream), computed once."""
    memo = {}

    def get(n, dead):
        if (n, dead) not in memo:
            alive = _alive(n, dead)
            memo[(n, dead)] = (alive, oracle.route(ragged, n, alive)[0])
        return memo[(n, dead)]

    return get


@pytest.fixture(scope="module")
def five_batches(ragged):
    """Five batches cut from the stream at '\\n's, sizes = 0, 1, 2, 3, 0 (mod 4)."""
    out, pos = [], 0
    for k in range(5):
        part = B.cut_at_newline(ragged[pos:], 400_000, 560_000, k % 4, mod=4)
        out.append(np.ascontiguousarray(part))
        pos += part.size
    assert [p.size % 4 for p in out] == [0, 1, 2, 3, 0] and all(p[-1] == 0x0A for p in out)
    return out


def _upload(torch, parts, poison=B.END_POISON, leads=None):
    """Each part between poison in a device tensor of its own; returns (tensors, device addresses)."""
    keep, addr = [], []
    for i, p in enumerate(parts):
        buf, off = B.embed(p, leads[i] if leads else 0, poison)
        t = torch.from_numpy(buf.copy()).to("cuda")
        keep.append(t)
        addr.append(t.data_ptr() + off)
        assert addr[-1] % 16 == (leads[i] if leads else 0)
    return keep, addr


@pytest.mark.parametrize("slots", ["nbytes", "lines"])
@pytest.mark.parametrize("n_shards,dead", [(64, 5), (3, 0)])
@pytest.mark.parametrize("G", [1, 2, 3, 8, 64])
def test_pack_by_owner_ragged(pkg, oracle, ragged, routed, torch_stream, G, n_shards, dead, slots):
    """sr_pack_by_owner over the whole stream: counts, records and all out_cap packed bytes."""
    import torch

    alive, recs = routed(n_shards, dead)
    nbytes = int(ragged.size)
    cap = nbytes if slots == "nbytes" else len(recs)
    assert _chunks(nbytes, cap) == (2 if slots == "nbytes" else 1)   # each run on its side of the threshold
    eb, er, ec = oracle.pack_by_owner(ragged, recs, G)
    with pkg.Router(n_shards, nbytes) as r:
        r.set_alive(alive)
        r.set_stream(torch_stream.cuda_stream)
        d_in = torch.from_numpy(ragged.copy()).to("cuda")
        d_rec = torch.full((cap,), -1, dtype=torch.int64, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
        r.route_device(d_in.data_ptr(), nbytes, d_rec.data_ptr(), cap, None, d_n.data_ptr())
        out_cap = pkg.pack_capacity(nbytes)
        d_pb = torch.full((out_cap,), 0xAB, dtype=torch.uint8, device="cuda")
        d_pr = torch.full((cap,), -1, dtype=torch.int64, device="cuda")
        d_cnt = torch.full((G, 2), -1, dtype=torch.int64, device="cuda")
        r.pack_by_owner(d_in.data_ptr(), nbytes, d_rec.data_ptr(), d_n.data_ptr(), cap, G,
                        d_pb.data_ptr(), out_cap, d_pr.data_ptr(), d_cnt.data_ptr())
        torch.cuda.synchronize()
        assert int(d_n.item()) == len(recs)
        assert np.array_equal(d_rec.cpu().numpy()[: len(recs)].view(pkg.RECORD_DTYPE), recs)
        assert d_cnt.cpu().numpy().tolist() == ec.tolist()
        got_r = d_pr.cpu().numpy()
        assert np.array_equal(got_r[: len(er)].view(pkg.RECORD_DTYPE), er)
        assert (got_r[len(er):] == -1).all()
        want = np.full(out_cap, 0xAB, dtype=np.uint8)
        want[: eb.size] = eb
        got_b = d_pb.cpu().numpy()
        if not np.array_equal(got_b, want):
            bad = np.nonzero(got_b != want)[0]
            raise AssertionError(f"{len(bad)} packed bytes differ, first at {int(bad[0])} of {eb.size} "
                                 f"(got {got_b[bad[0]]:#x}, want {want[bad[0]]:#x})")


def _many_setup(pkg, oracle, torch, r, parts, addr, n_shards, alive, cap):
    nb = len(parts)
    d_rec = torch.full((nb, cap), -1, dtype=torch.int64, device="cuda")
    d_n = torch.zeros(nb, dtype=torch.int64, device="cuda")
    batches = [(addr[b], int(p.size), d_rec[b].data_ptr(), cap, d_n[b].data_ptr()) for b, p in enumerate(parts)]
    r.route_device_many([(db, n, dr, mr, None, dn) for db, n, dr, mr, dn in batches])
    recs_list = [oracle.route(p, n_shards, alive)[0] for p in parts]
    return batches, recs_list, (d_rec, d_n)


@pytest.mark.parametrize("G,n_shards,dead,slots", [(1, 3, 0, "lines"), (3, 64, 5, "nbytes"), (8, 64, 5, "lines"),
                                                   (64, 64, 5, "nbytes")])
def test_pack_many_by_owner_ragged(pkg, oracle, five_batches, torch_stream, G, n_shards, dead, slots):
    """sr_pack_many_by_owner over five batches of sizes = 0..3 (mod 4), each at another base offset
    between poison."""
    import torch

    parts = five_batches
    alive = _alive(n_shards, dead)
    lines = [int((p == 0x0A).sum()) for p in parts]
    cap = max(p.size for p in parts) if slots == "nbytes" else max(lines)
    total = sum(int(p.size) for p in parts)
    assert _chunks(total, len(parts) * cap) == (2 if slots == "nbytes" else 1)
    keep, addr = _upload(torch, parts, leads=[0, 3, 6, 9, 13])
    out_cap = pkg.pack_capacity(total)
    d_pb = torch.full((out_cap,), 0xAB, dtype=torch.uint8, device="cuda")
    d_pr = torch.full((len(parts) * cap,), -1, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((G, 2), -1, dtype=torch.int64, device="cuda")
    with pkg.Router(n_shards, max(p.size for p in parts)) as r:
        r.set_alive(alive)
        r.set_stream(torch_stream.cuda_stream)
        batches, recs_list, _bufs = _many_setup(pkg, oracle, torch, r, parts, addr, n_shards, alive, cap)
        r.pack_many_by_owner(batches, G, d_pb.data_ptr(), out_cap, d_pr.data_ptr(), d_cnt.data_ptr())
        torch.cuda.synchronize()
    eb, er, ec = oracle.pack_many_by_owner(parts, recs_list, G)
    assert d_cnt.cpu().numpy().tolist() == ec.tolist()
    got_r = d_pr.cpu().numpy()
    assert np.array_equal(got_r[: len(er)].view(pkg.RECORD_DTYPE), er) and (got_r[len(er):] == -1).all()
    want = np.full(out_cap, 0xAB, dtype=np.uint8)
    want[: eb.size] = eb
    assert np.array_equal(d_pb.cpu().numpy(), want)


@pytest.mark.parametrize("G,own", [(1, 0), (3, 0), (3, 2), (8, 7), (64, 0), (64, 63)])
def test_pack_owner_split_ragged(pkg, oracle, five_batches, torch_stream, G, own):
    """sr_pack_owner_sizes + sr_pack_owner_scatter over the same batches: owner `own`'s chunk in its own
    buffers (0xCD beyond it), its range of the packed buffer untouched, the rest as the oracle packs it."""
    import torch

    parts, n_shards = five_batches, 64
    alive = _alive(n_shards, 5)
    cap = max(int((p == 0x0A).sum()) for p in parts)
    total = sum(int(p.size) for p in parts)
    keep, addr = _upload(torch, parts, leads=[1, 2, 7, 8, 15])
    out_cap = pkg.pack_capacity(total)
    d_pb = torch.full((out_cap,), 0xAB, dtype=torch.uint8, device="cuda")
    d_pr = torch.full((len(parts) * cap,), -1, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((G, 2), -1, dtype=torch.int64, device="cuda")
    with pkg.Router(n_shards, max(p.size for p in parts)) as r:
        r.set_alive(alive)
        r.set_stream(torch_stream.cuda_stream)
        batches, recs_list, _bufs = _many_setup(pkg, oracle, torch, r, parts, addr, n_shards, alive, cap)
        eb, er, ec = oracle.pack_many_by_owner(parts, recs_list, G)
        r.pack_owner_sizes(batches, G, d_cnt.data_ptr())
        torch.cuda.synchronize()
        assert d_cnt.cpu().numpy().tolist() == ec.tolist()
        ob = torch.full((int(ec[own, 1]) + 256,), 0xCD, dtype=torch.uint8, device="cuda")
        orr = torch.full((int(ec[own, 0]) + 8,), -1, dtype=torch.int64, device="cuda")
        r.pack_owner_scatter(batches, G, own, ob.data_ptr(), orr.data_ptr(), d_pb.data_ptr(), out_cap, d_pr.data_ptr())
        torch.cuda.synchronize()
    l0 = np.concatenate([[0], np.cumsum(ec[:, 0])]).astype(np.int64)
    b0 = np.concatenate([[0], np.cumsum(ec[:, 1])]).astype(np.int64)
    want_b = np.full(out_cap, 0xAB, dtype=np.uint8)
    want_b[: eb.size] = eb
    want_b[b0[own]: b0[own + 1]] = 0xAB            # nothing of the own chunk in the packed buffer
    assert np.array_equal(d_pb.cpu().numpy(), want_b)
    want_r = np.full(len(parts) * cap, -1, dtype=np.int64)
    want_r[: len(er)] = er.view(np.int64)
    want_r[l0[own]: l0[own + 1]] = -1
    assert np.array_equal(d_pr.cpu().numpy(), want_r)
    mine_b = ob.cpu().numpy()
    assert np.array_equal(mine_b[: ec[own, 1]], eb[b0[own]: b0[own + 1]]) and (mine_b[ec[own, 1]:] == 0xCD).all()
    mine_r = orr.cpu().numpy()
    assert np.array_equal(mine_r[: ec[own, 0]].view(pkg.RECORD_DTYPE), er[l0[own]: l0[own + 1]])
    assert (mine_r[ec[own, 0]:] == -1).all()


@pytest.mark.parametrize("G,own", [(1, None), (2, None), (3, None), (2, 0), (3, 2)])
def test_batch_end_and_base(pkg, oracle, torch_stream, G, own):
    """16 batches whose valid last line ends at the batch's last byte (one per nbytes mod 16, last lines
    of 6..1449 bytes), each at another base offset between 0xEE: the piece that crosses the batch's end
    must not bring a byte from past it."""
    import torch

    parts = B.end_batches()
    n_shards = 4
    leads = [(5 * i + 1) % 16 for i in range(16)]
    assert sorted(leads) == list(range(16)) and not any((p == 0xEE).any() for p in parts)
    keep, addr = _upload(torch, parts, poison=b"\xEE", leads=leads)
    cap = max(int((p == 0x0A).sum()) for p in parts)
    total = sum(int(p.size) for p in parts)
    out_cap = pkg.pack_capacity(total)
    d_pb = torch.full((out_cap,), 0xAB, dtype=torch.uint8, device="cuda")
    d_pr = torch.full((len(parts) * cap,), -1, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((G, 2), -1, dtype=torch.int64, device="cuda")
    with pkg.Router(n_shards, max(p.size for p in parts)) as r:
        r.set_stream(torch_stream.cuda_stream)
        batches, recs_list, _bufs = _many_setup(pkg, oracle, torch, r, parts, addr, n_shards, None, cap)
        eb, er, ec = oracle.pack_many_by_owner(parts, recs_list, G)
        if own is None:
            r.pack_many_by_owner(batches, G, d_pb.data_ptr(), out_cap, d_pr.data_ptr(), d_cnt.data_ptr())
        else:
            r.pack_owner_sizes(batches, G, d_cnt.data_ptr())
            ob = torch.full((int(ec[own, 1]) + 64,), 0xCD, dtype=torch.uint8, device="cuda")
            orr = torch.full((int(ec[own, 0]) + 1,), -1, dtype=torch.int64, device="cuda")
            r.pack_owner_scatter(batches, G, own, ob.data_ptr(), orr.data_ptr(), d_pb.data_ptr(), out_cap, d_pr.data_ptr())
        torch.cuda.synchronize()
    assert d_cnt.cpu().numpy().tolist() == ec.tolist()
    l0 = np.concatenate([[0], np.cumsum(ec[:, 0])]).astype(np.int64)
    b0 = np.concatenate([[0], np.cumsum(ec[:, 1])]).astype(np.int64)
    got_b = d_pb.cpu().numpy()
    got_r = d_pr.cpu().numpy()
    assert not (got_b == 0xEE).any(), f"poison in the packed bytes at {np.nonzero(got_b == 0xEE)[0][:8].tolist()}"
    want_b = np.full(out_cap, 0xAB, dtype=np.uint8)
    want_b[: eb.size] = eb
    want_r = np.full(len(parts) * cap, -1, dtype=np.int64)
    want_r[: len(er)] = er.view(np.int64)
    if own is not None:
        want_b[b0[own]: b0[own + 1]] = 0xAB
        want_r[l0[own]: l0[own + 1]] = -1
        mine_b, mine_r = ob.cpu().numpy(), orr.cpu().numpy()
        assert not (mine_b == 0xEE).any()
        assert np.array_equal(mine_b[: ec[own, 1]], eb[b0[own]: b0[own + 1]]) and (mine_b[ec[own, 1]:] == 0xCD).all()
        assert np.array_equal(mine_r[: ec[own, 0]].view(pkg.RECORD_DTYPE), er[l0[own]: l0[own + 1]])
        assert (mine_r[ec[own, 0]:] == -1).all()
    assert np.array_equal(got_b, want_b)
    assert np.array_equal(got_r, want_r)


@pytest.mark.parametrize("n,dead", [(1, 0), (3, 0), (64, 16)])
def test_route_pack_ragged(pkg, oracle, ragged, n, dead):
    """Route + MTU packing over every line length (the widest range of the packets' next() search)."""
    alive = _alive(n, dead)
    rng = np.random.default_rng(n)
    with pkg.Router(n, int(ragged.size)) as r:
        r.set_alive(alive)
        for fill in (None, rng.integers(0, 1451, n).tolist(), [1450] * n):
            _check_pack(pkg, oracle, ragged, n, alive, fill, r)
