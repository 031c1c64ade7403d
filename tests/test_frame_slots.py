"""Framing of datagrams left in their recvmmsg slots, the parts that need no GPU: the arena builder of the
device tests, sr_frame_slots_size against the CPU oracle, and the argument errors sr_frame_slots and
sr_route_pack_submit_slots report before they touch a device."""
from __future__ import annotations

import ctypes
import errno

import numpy as np
import pytest

import frame_slots as fs

SIZE_LENGTHS = [0, 1, 2, 15, 16, 17, 4094, 4095, 4096, 5000, 65535]


def _cases():
    for nl in (False, True):
        yield f"edges-nl{int(nl)}", fs.make_datagrams(SIZE_LENGTHS, 11, nl)
        yield f"shuffled-nl{int(nl)}", fs.make_datagrams(np.random.default_rng(5).permutation(SIZE_LENGTHS * 3), 12, nl)
    yield "just-newline", [b"\n", b"a", b"\n", b"\n"]
    yield "all-empty", [b"", b"", b""]
    yield "none", []


CASES = dict(_cases())


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("stride", [4096, 4111])
def test_builder_matches_oracle(oracle, name, stride):
    """What a reader of the arena sees, framed by the oracle, is the original datagrams framed by it."""
    dgrams = CASES[name]
    arena, lens = fs.build_arena(dgrams, stride)
    want, ends = fs.expected(oracle, dgrams)
    seen = fs.slot_bytes(arena, lens, stride)
    assert b"".join(oracle.frame(d) for d in seen) == want.tobytes()
    assert ends.size == len(dgrams) and (ends.size == 0 or int(ends[-1]) == want.size)
    assert all(int(lens[j]) == min(len(d), 65535) for j, d in enumerate(dgrams))


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("stride", [4096, 4097])
def test_frame_slots_size_matches_oracle(pkg, oracle, name, stride):
    dgrams = CASES[name]
    arena, lens = fs.build_arena(dgrams, stride)
    want, ends = fs.expected(oracle, dgrams)
    total, got_ends = pkg.frame_slots_size(arena, stride, lens, want_ends=True)
    assert total == want.size
    assert np.array_equal(got_ends, ends)
    assert pkg.frame_slots_size(arena, stride, lens) == want.size   # ends == NULL
    assert want.tobytes() == pkg.frame_datagrams(dgrams)            # and the two host framers agree


def test_argument_errors_without_a_device(pkg):
    L = pkg.lib()
    total = ctypes.c_uint64(7)
    lens = (ctypes.c_uint16 * 4)()
    slots = (ctypes.c_uint8 * 4096)()
    out = (ctypes.c_uint8 * 64)()

    def batch(stride=4096, count=1):
        return pkg.SrSlotBatch(ctypes.addressof(slots), stride, ctypes.addressof(lens), count, ctypes.addressof(out),
                               64, None, ctypes.addressof(total))

    # a null context, alone and together with a stride below the slot size and a count above SR_MAX_SLOTS
    for b in (batch(), batch(stride=4095), batch(count=pkg.SR_MAX_SLOTS + 1)):
        assert L.sr_frame_slots(None, ctypes.byref(b)) == -errno.EINVAL
    assert L.sr_frame_slots(None, None) == -errno.EINVAL
    assert L.sr_route_pack_submit_slots(None, 0, ctypes.addressof(slots), 4096, ctypes.addressof(lens), 1, None) \
        == -errno.EINVAL
    assert total.value == 7 and bytes(out) == bytes(64)
    assert pkg.SR_MAX_SLOTS == 65536
