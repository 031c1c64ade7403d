"""GPU: sr_route_pack_submit_slots against sr_route_pack_submit on the same datagrams framed by the host
(pkg.frame_datagrams), on two contexts. Everything a slot returns must be identical: sorted records,
packets, fills, the probed-dead bitmap, the trace records and hashes, the payload arena and its offsets."""
from __future__ import annotations

import errno

import numpy as np
import pytest

import frame_slots as fs

pytestmark = pytest.mark.gpu

MAX_BATCH = 192 << 10
STRIDE = 4096


def _datagrams(pkg, nbytes, seed):
    """Datagrams of statsd lines whose framed form is at most `nbytes` bytes: a generated stream cut at its
    datagram boundaries, a third of the datagrams without their final '\\n' (framing puts it back), and
    empty datagrams in between."""
    s = pkg.gen_stream(nbytes, [64, 256, 1024], seed=seed, p_invalid=0.1)
    rng = np.random.default_rng(seed)
    raw, pos, out = s.data.tobytes(), 0, []
    for n in s.dgram_lens.tolist():
        d = raw[pos: pos + n]
        pos += n
        out.append(d[:-1] if rng.random() < 1 / 3 else d)
        if rng.random() < 0.1:
            out.append(b"")
    return out


def _alive(n, dead):
    if not dead:
        return None
    a = np.ones(n, dtype=int)
    a[np.random.default_rng(n).choice(n, n // 4, replace=False)] = 0
    return a.tolist()


def _take(r, slot):
    res = r.route_pack_result(slot)
    return res + r.route_pack_trace(slot) + r.route_pack_payloads(slot)


def _same(a, b, label):
    names = ["sorted", "packets", "fill", "n_valid", "probed dead", "trace records", "trace hashes", "arena", "offsets"]
    assert len(a) == len(b) == len(names)
    for x, y, nm in zip(a, b, names):
        assert np.array_equal(x, y), f"{label}: {nm} differ"


@pytest.mark.parametrize("dead", [False, True], ids=["alive", "quarter-dead"])
@pytest.mark.parametrize("n", [4, 64])
def test_chained_batches_on_alternating_slots(pkg, n, dead):
    """Five chained batches, slots 0 and 1 alternating with two in flight, the third batch all empty
    datagrams; the first starts from given fills, the rest chain on the device."""
    batches = [_datagrams(pkg, MAX_BATCH // 2, 10 * n + i) for i in range(5)]
    batches[2] = [b""] * 7
    batches[4] = _datagrams(pkg, MAX_BATCH, 10 * n + 4)       # the largest: its framed size is max_batch_bytes
    alive = _alive(n, dead)
    fill0 = np.random.default_rng(n).integers(0, 1451, n).tolist()
    bufs = [pkg.HostBuffer(STRIDE * max(len(b) for b in batches)) for _ in range(2)]
    framed = [np.frombuffer(pkg.frame_datagrams(b), dtype=np.uint8) for b in batches]
    max_batch = framed[4].size
    assert framed[2].size == 0 and MAX_BATCH - 2048 < max_batch <= MAX_BATCH
    with pkg.Router(n, max_batch) as ra, pkg.Router(n, max_batch) as rb:
        for r in (ra, rb):
            if alive is not None:
                r.set_alive(alive)
            r.set_trace(True)
            r.set_payloads(True)
        lines = 0

        def submit(i):
            slot, fill = i % 2, fill0 if i == 0 else None
            arena, lens = fs.build_arena(batches[i], STRIDE)
            bufs[slot].array[:] = fs.POISON
            bufs[slot].array[: arena.size] = arena
            assert pkg.frame_slots_size(bufs[slot].array, STRIDE, lens) == framed[i].size
            ra.route_pack_submit(slot, framed[i], fill)
            rb.route_pack_submit_slots(slot, bufs[slot], STRIDE, lens, fill)

        submit(0)
        for i in range(1, 6):
            if i < 5:
                submit(i)
            want, got = _take(ra, (i - 1) % 2), _take(rb, (i - 1) % 2)
            _same(want, got, f"n={n} dead={dead} batch {i - 1}")
            lines += len(want[0])
        assert lines > 1000
        # a slot in flight is busy for both kinds of submission; one byte over max_batch_bytes is refused
        arena, lens = fs.build_arena(batches[4] + [b"\n"], STRIDE)
        big = pkg.HostBuffer(arena.size)
        big.array[:] = arena
        with pytest.raises(pkg.SrError) as e:
            rb.route_pack_submit_slots(0, big, STRIDE, lens)
        assert e.value.errno == errno.EINVAL
        rb.route_pack_submit_slots(0, big, STRIDE, lens[:-1])
        with pytest.raises(pkg.SrError) as e:
            rb.route_pack_submit_slots(0, big, STRIDE, lens[:-1])
        assert e.value.errno == errno.EBUSY
        ra.route_pack_submit(0, framed[4])
        _same(_take(ra, 0), _take(rb, 0), "after the refusals")
        big.close()
    for b in bufs:
        b.close()


def test_memory_without_a_device_address_is_refused(pkg):
    """Pageable memory has no device address: -EINVAL, and the context still works afterwards."""
    dgrams = [b"a.b.c:1|c", b"d.e.f:2|c\n"]
    arena, lens = fs.build_arena(dgrams, STRIDE, tail=64)
    with pkg.Router(4, 1 << 16) as r:
        with pytest.raises(pkg.SrError) as e:
            r.route_pack_submit_slots(0, arena.ctypes.data, STRIDE, lens)
        assert e.value.errno == errno.EINVAL
        buf = pkg.HostBuffer(arena.size)
        buf.array[:] = arena
        r.route_pack_submit_slots(0, buf, STRIDE, lens, [0, 0, 0, 0])
        srt, pk, fill, nv, _ = r.route_pack_result(0)
        assert len(srt) == 2 and nv == 2 and int(np.sum(fill)) == 20
        buf.close()
