"""GPU: sr_pack_payloads / sr_pack_payloads_many and the host-batch switch (sr_set_payloads), byte for
byte against the oracle: the arena is oracle.materialize's packets joined in descriptor order
(payload_expect.flat_expectation), the pending slots its new pending buffers. Every output buffer is
prefilled with a poison byte and compared whole, so a byte written where none belongs (the carry's
room, past the total, past a slot's fill) fails the test as surely as a wrong one."""
from __future__ import annotations

import errno

import numpy as np
import pytest

import byte_streams as B
import payload_expect as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ragged():
    return B.ragged_stream(1, 3 << 20)


def _alive(n, dead, seed=4):
    if not dead:
        return None
    if n == 1:
        return [0]
    rng = np.random.default_rng(seed)
    a = np.ones(n, dtype=int)
    a[rng.choice(n, max(n // 4, 2), replace=False)] = 0
    return a.tolist()


def _fills(n, rng):
    return {"none": [0] * n, "random": rng.integers(0, 1451, n).tolist(), "full": [1450] * n, "one": [1] * n}


# ---- 1. ragged bytes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dead", [False, True], ids=["alive", "dead"])
@pytest.mark.parametrize("n", [1, 7, 64])
def test_ragged_stream(pkg, oracle, ragged, torch_stream, n, dead):
    import torch

    rng = np.random.default_rng(100 + n)
    alive = _alive(n, dead)
    with pkg.Router(n, ragged.size) as r:
        if alive is not None:
            r.set_alive(alive)
        r.set_stream(torch_stream.cuda_stream)
        for name, fills in _fills(n, rng).items():
            e = X.Expect(oracle, ragged, n, alive, fills, X.random_pending(rng, fills))
            b = X.DeviceBatch(torch, pkg, ragged, n, fills, e.pending, max_records=e.n_lines)
            X.run(r, [b])
            torch.cuda.synchronize()
            X.check(b, e, label=f"n={n} dead={dead} fills={name}")


# ---- 2. packet extremes ------------------------------------------------------------------------------
EXTREMES = {
    "six": b"".join(b"%d:1|c\n" % (i % 10) for i in range(1000)),          # 241 lines a packet
    "longest": b"".join(b"%d" % i + b"x" * 1443 + b":1|c\n" for i in range(5)),   # 1449: one a packet
    "exact": b"".join(b"%d" % (i // 2) + b"z" * 719 + b":1|c\n" for i in range(8)),   # 2 x 725 = 1450
    "one_line": b"a:1|c\n",
    "no_valid": b"bad\nnocolon_line\n" + b"x" * 1500 + b"\n",
    "empty": b"",
    "mixed": b"bad\n" + b"k:1|c\n" * 500 + b"nocolon_line\n" + b"q" * 700 + b":1\n",
}


def test_packet_extremes(pkg, oracle, torch_stream):
    """Each shape with nothing pending, with full buffers (a carry-only flush: nlines = 0), with 1449
    pending bytes (the first line does not fit) and with fills that leave an exact fit, in one launch."""
    import torch

    n = 2
    rng = np.random.default_rng(7)
    specs = [(k, d, f) for k, d in EXTREMES.items() for f in ([0, 0], [1450, 1450], [1449, 1449], [725, 1444])]
    assert len(specs) <= pkg.SR_MAX_BATCHES_PER_LAUNCH
    exps = [X.Expect(oracle, d, n, None, f, X.random_pending(rng, f)) for _, d, f in specs]
    assert any(int(p["nlines"]) == 0 and int(p["carry"]) == 1450 for e in exps for p in e.packets)
    assert any(int(p["nlines"]) == 0 and int(p["carry"]) == 1449 for e in exps for p in e.packets)
    assert any(int(p["nlines"]) == 241 for e in exps for p in e.packets)
    assert any(int(p["carry"]) + int(p["length"]) == 1450 and int(p["nlines"]) for e in exps for p in e.packets)
    with pkg.Router(n, 1 << 16) as r:
        r.set_stream(torch_stream.cuda_stream)
        bs = [X.DeviceBatch(torch, pkg, d, n, f, e.pending) for (_, d, f), e in zip(specs, exps)]
        X.run(r, bs)
        torch.cuda.synchronize()
        for (k, _, f), b, e in zip(specs, bs, exps):
            X.check(b, e, label=f"{k} fills={f}")


# ---- 3. batch ends at odd addresses ------------------------------------------------------------------
def test_batches_end_at_odd_addresses(pkg, oracle, torch_stream):
    import torch

    n = 3
    rng = np.random.default_rng(9)
    ends = B.end_batches()
    fills = [rng.integers(0, 1451, n).tolist() for _ in ends]
    exps = [X.Expect(oracle, d, n, None, f, X.random_pending(rng, f, avoid=0xEE)) for d, f in zip(ends, fills)]
    with pkg.Router(n, 1 << 16) as r:
        r.set_stream(torch_stream.cuda_stream)
        bs = [X.DeviceBatch(torch, pkg, d, n, f, e.pending, lead=(2 * i + 1) % 16, in_poison=B.END_POISON)
              for i, (d, f, e) in enumerate(zip(ends, fills, exps))]
        assert all(b.in_ptr % 2 == 1 for b in bs)
        X.run(r, bs)
        torch.cuda.synchronize()
        for i, (b, e) in enumerate(zip(bs, exps)):
            X.check(b, e, label=f"end batch {i}")
            assert not (b.d_arena.cpu().numpy() == 0xEE).any(), i
            assert not (b.d_pout.cpu().numpy() == 0xEE).any(), i


# ---- 4. room mode ------------------------------------------------------------------------------------
def test_room_mode(pkg, oracle, ragged, torch_stream):
    """d_pend_in = NULL: every carry range keeps the prefill, everything else is the oracle's."""
    import torch

    n = 7
    rng = np.random.default_rng(21)
    data = B.cut_at_newline(ragged, 0, 1 << 20)
    with pkg.Router(n, data.size) as r:
        r.set_stream(torch_stream.cuda_stream)
        for name, fills in _fills(n, rng).items():
            e = X.Expect(oracle, data, n, None, fills, X.random_pending(rng, fills))
            b = X.DeviceBatch(torch, pkg, data, n, fills, None, max_records=e.n_lines)
            X.run(r, [b])
            torch.cuda.synchronize()
            X.check(b, e, room=True, label=f"room fills={name}")
            if name != "none":
                assert e.rooms
        out = torch.zeros(n * X.STRIDE, dtype=torch.uint8, device="cuda")
        with pytest.raises(pkg.SrError) as ei:
            r.pack_payloads_many([b.payload_tuple(pend_in=0, pend_out=out.data_ptr())])
        assert ei.value.errno == errno.EINVAL


# ---- 5. a device chain with alive toggles ------------------------------------------------------------
def test_device_chain_with_alive_toggles(pkg, oracle, torch_stream):
    """Twelve batches as in test_route_pack_chained_batches, fills and pending bytes living only on the
    device (two pending buffers used alternately): after every batch the flushed packets and the pending
    slots equal oracle.materialize's."""
    import torch

    n = 6
    rng = np.random.default_rng(3)
    pend_o, fill_o = {}, [0] * n
    P = [torch.full((n * X.STRIDE,), X.POISON, dtype=torch.uint8, device="cuda") for _ in range(2)]
    prev = None
    with pkg.Router(n, 1 << 18) as r:
        r.set_stream(torch_stream.cuda_stream)
        for k in range(12):
            alive = (rng.random(n) > 0.3).astype(int).tolist()
            s = pkg.gen_stream(int(rng.integers(1000, 1 << 18)), [6, 64, 300, 1449], seed=100 + k, p_invalid=0.05)
            r.set_alive(alive)
            e = X.Expect(oracle, s.data, n, alive, fill_o, pend_o)
            b = X.DeviceBatch(torch, pkg, s.data, n, None, None, max_records=max(e.n_lines, 1))
            if prev is not None:
                b.d_fin.copy_(prev.d_fout)   # the fills chain on the device too
            before = P[(k + 1) % 2].cpu().numpy().copy()
            r.route_pack_many([b.route_pack_tuple()])
            r.pack_payloads_many([b.payload_tuple(pend_in=P[k % 2].data_ptr(), pend_out=P[(k + 1) % 2].data_ptr())])
            torch.cuda.synchronize()
            X.check(b, e, label=f"chain batch {k}")
            # the flushed packets, cut out of the arena by the offsets
            arena, offs = b.d_arena.cpu().numpy(), e.offsets
            got = {}
            for i, p in enumerate(e.packets):
                if not int(p["open"]):
                    got.setdefault(int(p["shard"]), []).append(arena[int(offs[i]): int(offs[i + 1])].tobytes())
            assert got == e.flushed, k
            # the pending slots: the new pending bytes, nothing written at or past fill_out
            want = before
            for sh in range(n):
                nb_ = e.new_pending.get(sh, b"")
                want[sh * X.STRIDE: sh * X.STRIDE + len(nb_)] = np.frombuffer(nb_, dtype=np.uint8)
            assert np.array_equal(P[(k + 1) % 2].cpu().numpy(), want), k
            assert b.d_fout.cpu().numpy().view(np.uint16)[:n].tolist() == [int(f) for f in e.fill_out]
            pend_o, fill_o, prev = e.new_pending, [int(f) for f in e.fill_out], b


# ---- 6. many batches in one call ---------------------------------------------------------------------
def _many_batches(pkg, count, seed):
    """`count` batches of different sizes (mod 4 = 0, 1, 2, 3), among them an empty batch, a one-line
    batch and a batch of invalid lines only."""
    src = pkg.gen_stream(1 << 18, [6, 13, 64, 300, 1449], seed=seed, p_invalid=0.05).data
    out = []
    for i in range(count):
        if i == 3:
            out.append(np.zeros(0, np.uint8))
        elif i == 5:
            out.append(np.frombuffer(b"only:1|c\n", dtype=np.uint8))
        elif i == 9:
            out.append(np.frombuffer(b"bad\n" * 7 + b"nocolon_at_all\n", dtype=np.uint8))
        else:
            lo = 3000 + 1500 * i
            out.append(B.cut_at_newline(src[i * 97:], lo, lo + 30000, i % 4, mod=4).copy())
    return out


def test_many_batches_in_one_call(pkg, oracle, torch_stream):
    import torch

    n, count = 5, 32
    rng = np.random.default_rng(31)
    alive = [1, 1, 0, 1, 1]
    datas = _many_batches(pkg, count, 0x6A)
    assert {d.size % 4 for d in datas} == {0, 1, 2, 3}
    fills = [rng.integers(0, 1451, n).tolist() for _ in datas]
    exps = [X.Expect(oracle, d, n, alive, f, X.random_pending(rng, f)) for d, f in zip(datas, fills)]
    with pkg.Router(n, 1 << 18) as r:
        r.set_alive(alive)
        r.set_stream(torch_stream.cuda_stream)
        bs = [X.DeviceBatch(torch, pkg, d, n, f, e.pending) for d, f, e in zip(datas, fills, exps)]
        X.run(r, bs)
        torch.cuda.synchronize()
        for i, (b, e) in enumerate(zip(bs, exps)):
            X.check(b, e, label=f"batch {i} of {count}")


# ---- 7. many downstreams -----------------------------------------------------------------------------
def test_many_downstreams(pkg, oracle, torch_stream):
    """n = 4096 and a 64 KiB batch: most downstreams have no descriptor, so their pending bytes pass
    through, except those the batch probed dead, whose slot is not written."""
    import torch

    n = 4096
    rng = np.random.default_rng(41)
    alive = (rng.random(n) > 0.25).astype(int).tolist()
    data = pkg.gen_stream(1 << 16, [64, 300], seed=0x77, p_invalid=0.05).data
    fills = rng.integers(0, 1451, n).tolist()
    e = X.Expect(oracle, data, n, alive, fills, X.random_pending(rng, fills))
    with_desc = set(e.packets["shard"].tolist())
    assert len(with_desc) < n // 2 and len(e.probed) > 0
    assert any(fills[s] and s not in with_desc for s in e.probed)          # a drop
    assert any(fills[s] and s not in with_desc and int(e.fill_out[s]) == fills[s] for s in range(n))   # a pass-through
    with pkg.Router(n, 1 << 16) as r:
        r.set_alive(alive)
        r.set_stream(torch_stream.cuda_stream)
        b = X.DeviceBatch(torch, pkg, data, n, fills, e.pending, max_records=e.n_lines)
        X.run(r, [b])
        torch.cuda.synchronize()
        X.check(b, e, label="4096 downstreams")


# ---- 8. no room --------------------------------------------------------------------------------------
def test_no_room(pkg, oracle, torch_stream):
    import torch

    n = 4
    rng = np.random.default_rng(51)
    data = pkg.gen_stream(1 << 16, [6, 64, 300, 1449], seed=0x88, p_invalid=0.05).data
    fills = rng.integers(0, 1451, n).tolist()
    e = X.Expect(oracle, data, n, None, fills, X.random_pending(rng, fills))
    with pkg.Router(n, 1 << 16) as r:
        r.set_stream(torch_stream.cuda_stream)
        # an arena one byte short: *d_total says so, nothing at or past the capacity is written
        b = X.DeviceBatch(torch, pkg, data, n, fills, e.pending, payload_cap=e.total - 1)
        X.run(r, [b])
        torch.cuda.synchronize()
        assert int(b.d_total.item()) == e.total > b.pcap
        X.check(b, e, label="payload_cap = total - 1")
        # descriptor room one short: d_counts[0] says so, the written descriptors' packets are right
        b = X.DeviceBatch(torch, pkg, data, n, fills, e.pending, max_packets=len(e.packets) - 1)
        X.run(r, [b])
        torch.cuda.synchronize()
        assert int(b.d_counts[0].item()) == len(e.packets) > b.mp
        X.check(b, e, label="max_packets = n_packets - 1")
        # and with enough room afterwards
        b = X.DeviceBatch(torch, pkg, data, n, fills, e.pending)
        X.run(r, [b])
        torch.cuda.synchronize()
        X.check(b, e, label="enough room")


# ---- 9. stream capture -------------------------------------------------------------------------------
def test_stream_capture(pkg, oracle, torch_stream):
    """One warm call, then route + pack + payloads of 8 batches captured once and replayed twice, the
    input bytes replaced in between."""
    import torch

    n, count = 6, 8
    rng = np.random.default_rng(61)
    alive = None   # (the all-alive launch is the one the benchmark captures)
    first = _many_batches(pkg, count, 0x6B)
    other = pkg.gen_stream(1 << 18, [7, 64, 300, 1449], seed=0x6C, p_invalid=0.05).data
    second = []
    for d in first:   # other bytes of the same sizes
        o = other[: d.size].copy()
        if o.size:
            o[-1] = B.NL
        second.append(o)
    fills = [rng.integers(0, 1451, n).tolist() for _ in first]
    pend = [X.random_pending(rng, f) for f in fills]
    with pkg.Router(n, 1 << 18) as r:
        # a fixed lane layout: under SR_LAYOUT_AUTO the warm call is the context's first launch, a probe in
        # the segment layout, and the captured launch could take another layout, whose packing needs scratch
        # the warm call did not allocate
        r.set_layout(pkg.SR_LAYOUT_UNIFORM)
        r.set_stream(torch_stream.cuda_stream)
        bs = [X.DeviceBatch(torch, pkg, d, n, f, p) for d, f, p in zip(first, fills, pend)]
        X.run(r, bs)   # warm: the packing's scratch is allocated outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch_stream):
            X.run(r, bs)
        for datas in (first, second):
            for b, d in zip(bs, datas):
                b.refill()
                if d.size:
                    b.d_in.copy_(torch.from_numpy(d.copy()))
            g.replay()
            torch.cuda.synchronize()
            for i, (b, d, f, p) in enumerate(zip(bs, datas, fills, pend)):
                X.check(b, X.Expect(oracle, d, n, alive, f, p), label=f"replay batch {i}")


# ---- 10. host-batch path -----------------------------------------------------------------------------
def _check_host(got, e, label):
    arena, offs = got
    assert np.array_equal(offs, e.offsets), f"{label}: offsets"
    keep = np.ones(e.total, dtype=bool)
    for lo, hi in e.rooms:
        keep[lo:hi] = False
    want = np.frombuffer(e.arena, dtype=np.uint8)
    assert arena.size == e.total and np.array_equal(arena[keep], want[keep]), f"{label}: arena outside the carry room"


def test_host_batch_path(pkg, oracle):
    """The 14 double-buffered submissions of test_route_pack_submit_double_buffered with set_payloads(True):
    each slot's arena and offsets equal the oracle's outside the carry room, the ordinary results are
    unchanged; with the switch off the accessor gives -EBUSY."""
    from test_gpu_mtu import assert_pack_equal

    n = 7
    rng = np.random.default_rng(11)
    fill_o = [0] * n
    with pkg.Router(n, 1 << 18) as r:
        r.route_pack_submit(0, b"k:1|c\n")
        r.route_pack_result(0)
        with pytest.raises(pkg.SrError) as ei:   # submitted with the switch off
            r.route_pack_payloads(0)
        assert ei.value.errno == errno.EBUSY
        r.set_payloads(True)
        fill_o = [0] * n   # (the host sets the fills at batch 0)
        inflight = None

        def take(fl):
            slot, (want, e) = fl
            assert_pack_equal(r.route_pack_result(slot), want)
            _check_host(r.route_pack_payloads(slot), e, f"slot {slot}")

        for b in range(14):
            alive = (rng.random(n) > 0.3).astype(int).tolist()
            s = pkg.gen_stream(int(rng.integers(1, 1 << 18)), [6, 64, 300, 1449], seed=300 + b, p_invalid=0.05)
            host_fill = None
            if b in (0, 6):
                host_fill = rng.integers(0, 1451, n).tolist()
                if inflight is not None:
                    take(inflight)
                    inflight = None
                fill_o = host_fill
            r.set_alive(alive)
            slot = b % 2
            r.route_pack_submit(slot, s.data, host_fill)
            with pytest.raises(pkg.SrError) as ei:   # in flight
                r.route_pack_payloads(slot)
            assert ei.value.errno == errno.EBUSY
            e = X.Expect(oracle, s.data, n, alive, fill_o, {k: bytes(int(f)) for k, f in enumerate(fill_o)})
            fill_o = [int(f) for f in e.fill_out]
            if inflight is not None:
                take(inflight)
            inflight = (slot, ((e.sorted, e.packets, e.fill_out, e.n_valid, e.probed), e))
        take(inflight)
        # slot 2: the synchronous call
        srt, pk, fo, nv, pr = r.route_pack(s.data, fill_o)
        e = X.Expect(oracle, s.data, n, alive, fill_o, {k: bytes(int(f)) for k, f in enumerate(fill_o)})
        assert np.array_equal(pk.view(np.uint8), e.packets.view(np.uint8))
        _check_host(r.route_pack_payloads(2), e, "slot 2")
        r.set_payloads(False)
        r.route_pack_submit(0, s.data, fill_o)
        r.route_pack_result(0)
        with pytest.raises(pkg.SrError) as ei:
            r.route_pack_payloads(0)
        assert ei.value.errno == errno.EBUSY


# ---- 11. argument errors -----------------------------------------------------------------------------
def test_argument_errors(pkg, oracle, torch_stream):
    import torch

    n = 3
    data = b"k:1|c\n" * 50
    fills = [5, 0, 9]
    e = X.Expect(oracle, data, n, None, fills, X.random_pending(np.random.default_rng(1), fills))
    with pkg.Router(n, 1 << 12) as r:
        r.set_stream(torch_stream.cuda_stream)
        b = X.DeviceBatch(torch, pkg, data, n, fills, e.pending)
        good = list(b.payload_tuple())
        names = ["d_bytes", "nbytes", "d_sorted", "max_records", "d_packets", "max_packets", "d_counts", "d_fill_out",
                 "d_pend_in", "d_pend_out", "d_payload", "payload_cap", "d_offsets", "d_total"]

        def bad(**kw):
            t = list(good)
            for k, v in kw.items():
                t[names.index(k)] = v
            return tuple(t)

        cases = {
            "no bytes": bad(d_bytes=0), "no sorted": bad(d_sorted=0), "no packets": bad(d_packets=0),
            "no counts": bad(d_counts=0), "no fill_out": bad(d_fill_out=0), "no payload": bad(d_payload=0),
            "no offsets": bad(d_offsets=0), "no total": bad(d_total=0),
            "pend_out without pend_in": bad(d_pend_in=0),
            "pend_out == pend_in": bad(d_pend_out=good[names.index("d_pend_in")]),
        }
        for what, t in cases.items():
            for call in (lambda: r.pack_payloads_many([t]), lambda: r.pack_payloads(t)):
                with pytest.raises(pkg.SrError) as ei:
                    call()
                assert ei.value.errno == errno.EINVAL, what
        lib, arr = pkg.lib(), r.payload_batches([tuple(good)] * 33)
        assert lib.sr_pack_payloads_many(r.handle, arr, 0) == -errno.EINVAL
        assert lib.sr_pack_payloads_many(r.handle, arr, 33) == -errno.EINVAL
        assert lib.sr_pack_payloads_many(r.handle, None, 1) == -errno.EINVAL
        assert lib.sr_pack_payloads_many(None, arr, 1) == -errno.EINVAL
        assert lib.sr_pack_payloads(r.handle, None) == -errno.EINVAL
        assert lib.sr_set_payloads(None, 1) == -errno.EINVAL
        # nothing ran: the good batch still does
        X.run(r, [b])
        torch.cuda.synchronize()
        X.check(b, e, label="after the refused calls")
