"""GPU: the log text of the host-memory path (sr_set_logtext, sr_route_pack_set_prefix / _set_ends,
sr_route_pack_logtext) on slots 0, 1 and 2 and on the slots form, against tests/log_expect.py over the CPU
oracle's records; the staging that lasts one submission, the -EBUSY rules and a batch that overflows its
arena."""
from __future__ import annotations

import errno

import numpy as np
import pytest

import frame_slots as fs
import log_expect as L

pytestmark = pytest.mark.gpu

PFX = (b"2026-01-01 00:00:00 [TRACE] th0 ", b"W:")
N, ALIVE = 4, [1, 0, 1, 1]
DGRAMS = [b"a.b.c:1|c\nnocolon-here\n", b"", b"x\n", b"::1|cc\n\xff\xfe:1|c", b"y" * 1500, b"cut\0here:1|c\nq:2|c"] + \
    [b"m%d.n:%d|c\n" % (i, i) * (1 + i % 7) for i in range(120)]


def _errno(pkg, fn, *a):
    with pytest.raises(pkg.SrError) as e:
        fn(*a)
    return e.value.errno


@pytest.fixture(scope="module")
def batch(oracle):
    framed = [oracle.frame(d) for d in DGRAMS]
    data = b"".join(framed)
    ends = np.cumsum([len(f) for f in framed]).astype(np.uint32)
    recs, hs, cnt = oracle.route(data, N, ALIVE)
    assert cnt > 256
    return data, ends, recs[:cnt], hs[:cnt]


def _want(batch, level, ends=True, prefixes=PFX, max_msg=2047):
    data, e, recs, hs = batch
    return L.expect(data, recs, hs, e if ends else None, N, level, prefixes, max_msg)


def _same(got, want, label):
    text, total, offs, lv, ok = got
    assert ok, label
    assert total == len(want[0]) and text == want[0], label
    assert np.array_equal(offs, want[1]) and np.array_equal(lv, want[2]), label


@pytest.mark.parametrize("level", [0, 3])
def test_slots_0_1_2_and_the_slots_form(pkg, batch, level):
    data, ends, recs, hs = batch
    arena, lens = fs.build_arena(DGRAMS, 4096)
    hb = pkg.HostBuffer(arena.size)
    hb.array[:] = arena
    with pkg.Router(N, 1 << 17) as r:
        r.set_alive(ALIVE)
        # the switch is off: nothing to stage, nothing to take
        assert _errno(pkg, r.route_pack_set_prefix, 0, b"x", b"y") == errno.EINVAL
        assert _errno(pkg, r.route_pack_set_ends, 0, ends) == errno.EINVAL
        r.route_pack_submit(0, data, [0] * N)
        base = r.route_pack_result(0)
        assert _errno(pkg, r.route_pack_logtext, 0) == errno.EBUSY
        r.set_logtext(level, 0, 2047)
        for slot in (0, 1):
            r.route_pack_set_prefix(slot, *PFX)
            r.route_pack_set_ends(slot, ends)
            r.route_pack_submit(slot, data, [0] * N)
            for fn, a in ((r.route_pack_set_prefix, (slot, b"x", b"y")), (r.route_pack_set_ends, (slot, ends)),
                          (r.route_pack_logtext, (slot,)), (r.set_logtext, (level, 0, 0))):
                assert _errno(pkg, fn, *a) == errno.EBUSY, fn
            res = r.route_pack_result(slot)
            for x, y in zip(res, base):
                assert np.array_equal(x, y)   # the routed batch is what it is without the switch
            _same(r.route_pack_logtext(slot), _want(batch, level), f"slot {slot}")
            # staged for one submission: the next one has no prefix and no "got packet"
            r.route_pack_submit(slot, data, [0] * N)
            r.route_pack_result(slot)
            _same(r.route_pack_logtext(slot), _want(batch, level, ends=False, prefixes=(b"", b"")), f"slot {slot} unstaged")
        # slot 2: sr_route_pack_batch
        r.route_pack_set_prefix(2, *PFX)
        r.route_pack_set_ends(2, ends)
        r.route_pack(data, [0] * N)
        _same(r.route_pack_logtext(2), _want(batch, level), "slot 2")
        # the slots form takes its ends from the frame kernels
        for slot in (1, 0):
            r.route_pack_set_prefix(slot, *PFX)
            r.route_pack_submit_slots(slot, hb, 4096, lens, [0] * N)
            r.route_pack_result(slot)
            _same(r.route_pack_logtext(slot), _want(batch, level), f"slots form, slot {slot}")
        # an empty batch has an empty log
        r.route_pack_submit(0, b"", [0] * N)
        r.route_pack_result(0)
        text, total, offs, lv, ok = r.route_pack_logtext(0)
        assert ok and total == 0 and text == b"" and offs.tolist() == [0] and lv.size == 0
        # the trace outputs stay available next to the text
        r.set_trace(True)
        r.route_pack_set_ends(1, ends)
        r.route_pack_submit(1, data, [0] * N)
        r.route_pack_result(1)
        trecs, ths = r.route_pack_trace(1)[:2]
        assert np.array_equal(trecs, recs) and np.array_equal(ths, hs)
        _same(r.route_pack_logtext(1), _want(batch, level, prefixes=(b"", b"")), "with trace")
        r.set_trace(False)
        # off again: the slot's next batch has no text
        r.set_logtext(None)
        r.route_pack_submit(1, data, [0] * N)
        r.route_pack_result(1)
        assert _errno(pkg, r.route_pack_logtext, 1) == errno.EBUSY
    hb.close()


def test_overflowing_batch_and_bad_max_msg(pkg, batch):
    data, ends, recs, hs = batch
    want = _want(batch, 0, max_msg=0)
    with pkg.Router(N, 1 << 17) as r:
        r.set_alive(ALIVE)
        for cap in (1000, len(want[0]) - 1):
            r.set_logtext(0, cap, 0)
            r.route_pack_set_prefix(0, *PFX)
            r.route_pack_set_ends(0, ends)
            r.route_pack_submit(0, data, [0] * N)
            r.route_pack_result(0)
            text, total, offs, lv, ok = r.route_pack_logtext(0)
            assert not ok and total == len(want[0]) and text == want[0][:cap]
            k = lv.size
            assert np.array_equal(offs, want[1][: k + 1]) and np.array_equal(lv, want[2][:k])
        r.set_logtext(0, len(want[0]), 0)
        r.route_pack_set_prefix(0, *PFX)
        r.route_pack_set_ends(0, ends)
        r.route_pack_submit(0, data, [0] * N)
        r.route_pack_result(0)
        _same(r.route_pack_logtext(0), want, "exact room")
        # max_msg must clear both staged prefixes: the submission is refused, the slot stays free
        r.set_logtext(0, 0, 32)
        r.route_pack_set_prefix(0, *PFX)
        assert _errno(pkg, r.route_pack_submit, 0, data, [0] * N) == errno.EINVAL
        r.set_logtext(0, 0, 33)
        r.route_pack_set_prefix(0, *PFX)
        r.route_pack_set_ends(0, ends)
        r.route_pack_submit(0, data, [0] * N)
        r.route_pack_result(0)
        _same(r.route_pack_logtext(0), _want(batch, 0, max_msg=33), "max_msg 33")
        assert _errno(pkg, r.set_logtext, 4) == errno.EINVAL
        assert _errno(pkg, r.route_pack_set_prefix, 3, b"", b"") == errno.EINVAL
        assert _errno(pkg, r.route_pack_set_prefix, 0, b"p" * 257, b"") == errno.EINVAL
