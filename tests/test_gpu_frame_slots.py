"""GPU: sr_frame_slots, datagrams framed on the device from their recvmmsg slots, byte for byte against the
CPU oracle (oracle.frame over the datagrams themselves; frame_slots.expected). Every output (the framed
batch, the ends, the total) is prefilled with a poison byte, lies between 64 guard bytes and is compared
whole, so a byte written where none belongs (past the total, past the capacity, into a neighbour's piece)
fails the test as surely as a wrong one."""
from __future__ import annotations

import ctypes
import errno

import numpy as np
import pytest

import frame_slots as fs

pytestmark = pytest.mark.gpu

GUARD = 64
OUT_POISON = 0xCD
SPAN = 1024   # datagrams per workgroup of frame_lens_kernel (kFrameSpan): the scan's boundary


@pytest.fixture(scope="module")
def router(pkg):
    with pkg.Router(4, 1 << 16) as r:
        yield r


class Framed:
    """One sr_frame_slots call on device buffers and the comparison of everything it may have written."""

    def __init__(self, torch, arena, lens, stride, *, src_mis=0, dst_mis=0, cap=None, total=None, want_ends=True,
                 d_slots=None):
        self.torch = torch
        self.count = int(len(lens))
        self.stride = stride
        self.cap = int(total if cap is None else cap)
        self.dst_mis = dst_mis
        if d_slots is None:
            self.src = torch.empty(arena.size + src_mis + 16, dtype=torch.uint8, device="cuda")
            if arena.size:
                self.src[src_mis: src_mis + arena.size].copy_(torch.from_numpy(arena))
            self.d_slots = self.src.data_ptr() + src_mis
        else:
            self.d_slots = d_slots
        self.lens = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint16).view(np.int16).copy()).cuda()
        self.out = torch.empty(GUARD + dst_mis + self.cap + GUARD, dtype=torch.uint8, device="cuda")
        self.ends = torch.empty(GUARD + 4 * self.count + GUARD, dtype=torch.uint8, device="cuda") if want_ends else None
        self.total = torch.empty(GUARD + 8 + GUARD, dtype=torch.uint8, device="cuda")
        assert self.out.data_ptr() % 16 == 0
        self.poison()

    def poison(self):
        for t in (self.out, self.ends, self.total):
            if t is not None:
                t.fill_(OUT_POISON)

    def run(self, r):
        r.frame_slots(self.d_slots, self.stride, self.lens.data_ptr(), self.count,
                      self.out.data_ptr() + GUARD + self.dst_mis, self.cap,
                      self.ends.data_ptr() + GUARD if self.ends is not None else None, self.total.data_ptr() + GUARD)

    def check(self, want, want_ends, label=""):
        self.torch.cuda.synchronize()
        total = np.full(GUARD + 8 + GUARD, OUT_POISON, dtype=np.uint8)
        total[GUARD: GUARD + 8] = np.frombuffer(np.uint64(want.size).tobytes(), dtype=np.uint8)
        assert np.array_equal(self.total.cpu().numpy(), total), f"{label}: total"
        w = min(want.size, self.cap)
        out = np.full(self.out.numel(), OUT_POISON, dtype=np.uint8)
        out[GUARD + self.dst_mis: GUARD + self.dst_mis + w] = want[:w]
        got = self.out.cpu().numpy()
        if not np.array_equal(got, out):
            bad = np.flatnonzero(got != out)
            raise AssertionError(f"{label}: framed bytes differ at {bad[:8].tolist()} of {out.size} "
                                 f"(first framed byte at {GUARD + self.dst_mis}, {w} written)")
        if self.ends is not None:
            e = np.full(self.ends.numel(), OUT_POISON, dtype=np.uint8)
            e[GUARD: GUARD + 4 * self.count] = np.frombuffer(want_ends.astype("<u4").tobytes(), dtype=np.uint8)
            assert np.array_equal(self.ends.cpu().numpy(), e), f"{label}: ends"


def _frame(torch, r, oracle, dgrams, stride=4096, label="", **kw):
    arena, lens = fs.build_arena(dgrams, stride)
    want, ends = fs.expected(oracle, dgrams)
    caps = kw.pop("caps", [0])             # the capacity as a difference from the total, or "zero"
    ends_modes = kw.pop("ends_modes", (True, False))
    for cap in caps:
        room = 0 if cap == "zero" else max(want.size + cap, 0)
        for want_ends in ends_modes:
            f = Framed(torch, arena, lens, stride, cap=room, want_ends=want_ends, **kw)
            f.run(r)
            f.check(want, ends, f"{label} cap={cap} ends={want_ends}")
    return want.size


# ---- 1. the lengths at every edge ----------------------------------------------------------------------
@pytest.mark.parametrize("nl", [False, True], ids=["no-newline", "newline"])
@pytest.mark.parametrize("order", ["cycled", "shuffled"])
def test_edge_lengths(pkg, oracle, router, torch_stream, order, nl):
    import torch

    router.set_stream(torch_stream.cuda_stream)
    lengths = fs.EDGE_LENGTHS * 5
    if order == "shuffled":
        lengths = np.random.default_rng(17).permutation(lengths).tolist()
    _frame(torch, router, oracle, fs.make_datagrams(lengths, 3, nl), label=f"{order} nl={nl}")


def test_mixed_newlines(pkg, oracle, router, torch_stream):
    import torch

    router.set_stream(torch_stream.cuda_stream)
    rng = np.random.default_rng(23)
    lengths = rng.permutation(fs.EDGE_LENGTHS * 4).tolist()
    a, b = fs.make_datagrams(lengths, 4, False), fs.make_datagrams(lengths, 5, True)
    _frame(torch, router, oracle, [x if rng.random() < 0.5 else y for x, y in zip(a, b)], label="mixed")


# ---- 2. special batches ----------------------------------------------------------------------------------
def test_special_batches(pkg, oracle, router, torch_stream):
    import torch

    router.set_stream(torch_stream.cuda_stream)
    assert _frame(torch, router, oracle, [b""] * 40, label="all empty") == 0
    for d in (b"", b"\n", b"x", b"0123456789abcdefg", bytes(range(48, 58)) * 500):
        _frame(torch, router, oracle, [d], label=f"count 1, {len(d)} bytes")
    # 1-byte datagrams: a 16-byte piece spans 16 of them ("\n" stays 1 byte, anything else becomes 2)
    assert _frame(torch, router, oracle, [b"\n"] * 200, label="only newlines") == 200
    assert _frame(torch, router, oracle, [b"x"] * 200, label="only x") == 400
    _frame(torch, router, oracle, [b"\n", b"x", b"", b"\n", b"\n", b"y"] * 40, label="1-byte mix")
    # count == 0 writes the total and nothing else
    f = Framed(torch, np.zeros(0, np.uint8), np.zeros(0, np.uint16), 4096, total=0, cap=32)
    f.run(router)
    f.check(np.zeros(0, np.uint8), np.zeros(0, np.uint32), "count 0")


# ---- 3. every scan boundary --------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [63, 64, 65, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 3])
def test_counts_around_scan_boundaries(pkg, oracle, router, torch_stream, count):
    import torch

    router.set_stream(torch_stream.cuda_stream)
    lengths = [[0, 1, 2, 3, 17, 40, 16][i % 7] for i in range(count)]
    rng = np.random.default_rng(count)
    a, b = fs.make_datagrams(lengths, count, False), fs.make_datagrams(lengths, count + 1, True)
    _frame(torch, router, oracle, [x if rng.random() < 0.5 else y for x, y in zip(a, b)], label=f"count {count}")


def test_max_slots_of_tiny_datagrams(pkg, oracle, router, torch_stream):
    import torch

    router.set_stream(torch_stream.cuda_stream)
    count = pkg.SR_MAX_SLOTS
    rng = np.random.default_rng(65536)
    lengths = rng.integers(1, 4, count).tolist()
    a, b = fs.make_datagrams(lengths, 1, False), fs.make_datagrams(lengths, 2, True)
    pick = rng.random(count) < 0.5
    _frame(torch, router, oracle, [x if p else y for x, y, p in zip(a, b, pick)], label="65536 slots",
           ends_modes=(True,))


# ---- 4. alignments ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [4096, 4097, 4111])
def test_alignments(pkg, oracle, router, torch_stream, stride):
    import torch

    router.set_stream(torch_stream.cuda_stream)
    rng = np.random.default_rng(stride)
    lengths = rng.permutation(fs.EDGE_LENGTHS * 2).tolist()
    a, b = fs.make_datagrams(lengths, 8, False), fs.make_datagrams(lengths, 9, True)
    dgrams = [x if rng.random() < 0.5 else y for x, y in zip(a, b)]
    for dst_mis in (0, 1, 4, 15):
        for src_mis in (0, 1, 3):
            _frame(torch, router, oracle, dgrams, stride, label=f"stride {stride} dst+{dst_mis} src+{src_mis}",
                   dst_mis=dst_mis, src_mis=src_mis, ends_modes=(True,))


# ---- 5. capacity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst_mis", [0, 5])
def test_capacity_cuts_the_batch(pkg, oracle, router, torch_stream, dst_mis):
    """cap = total, total - 1, total - 17 and 0: nothing at or past it is written and d_total still says the
    need."""
    import torch

    router.set_stream(torch_stream.cuda_stream)
    dgrams = fs.make_datagrams([100, 0, 1, 33, 1449, 7, 16, 16, 1, 1, 1, 250], 31, False)
    _frame(torch, router, oracle, dgrams, label="caps", caps=[0, -1, -17, "zero"], dst_mis=dst_mis)


# ---- 6. 64-bit source addresses ------------------------------------------------------------------------------------
def test_slot_offsets_past_4_gib(pkg, oracle, router, torch_stream):
    """stride 70000 with 65536 slots: j * stride passes 2^32 between slots 61356 and 61357. The arena is
    allocated but not initialised; only four slots hold datagrams."""
    import torch

    router.set_stream(torch_stream.cuda_stream)
    stride, count = 70000, pkg.SR_MAX_SLOTS
    used = [0, 61356, 61357, 65535]
    assert used[1] * stride < 1 << 32 <= used[2] * stride
    four = fs.make_datagrams([1449, 4095, 300, 17], 64, False)
    arena = torch.empty((count - 1) * stride + 4096, dtype=torch.uint8, device="cuda")
    lens = np.zeros(count, dtype=np.uint16)
    dgrams = [b""] * count
    for j, d in zip(used, four):
        arena[j * stride: j * stride + len(d)].copy_(torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()))
        lens[j] = len(d)
        dgrams[j] = d
    want = np.frombuffer(b"".join(oracle.frame(d) for d in four), dtype=np.uint8)
    ends = np.zeros(count, dtype=np.uint32)
    pos = 0
    for j in range(4):
        pos += len(oracle.frame(four[j]))
        ends[used[j]: used[j + 1] if j < 3 else count] = pos
    f = Framed(torch, None, lens, stride, total=want.size, d_slots=arena.data_ptr())
    f.run(router)
    f.check(want, ends, "4.6 GB arena")
    del arena


# ---- 7. graph capture ------------------------------------------------------------------------------------------------
def test_captured_call_replays_on_changed_slots(pkg, oracle, router, torch_stream):
    import torch

    router.set_stream(torch_stream.cuda_stream)
    lengths = [[64, 1, 0, 1400, 17][i % 5] for i in range(SPAN + 40)]
    first = fs.make_datagrams(lengths, 41, False)
    arena, lens = fs.build_arena(first, 4096)
    want, ends = fs.expected(oracle, first)
    f = Framed(torch, arena, lens, 4096, total=want.size + 4096)
    f.run(router)   # eager: the context's scan scratch is allocated outside the capture
    f.check(want, ends, "eager")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch_stream):
        f.run(router)
    # other contents in the same slots, other lengths too: some datagrams now end in '\n', some are empty
    second = fs.make_datagrams([[1, 64, 1400, 0, 16][i % 5] for i in range(SPAN + 40)], 42, True)
    for label, dgrams in (("replay 1", second), ("replay 2", first)):
        arena, lens = fs.build_arena(dgrams, 4096, tail=0)
        want, ends = fs.expected(oracle, dgrams)
        f.src.fill_(fs.POISON)
        f.src[: arena.size].copy_(torch.from_numpy(arena))
        f.lens.copy_(torch.from_numpy(lens.view(np.int16).copy()))
        f.poison()
        g.replay()
        f.check(want, ends, label)


# ---- 8. argument errors on a live context ------------------------------------------------------------------------------
def test_argument_errors(pkg, router, torch_stream):
    import torch

    router.set_stream(torch_stream.cuda_stream)
    buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    ok = dict(d_slots=p, stride=4096, d_lens=p + 4096, count=1, d_bytes=p + 4200, cap=64, d_ends=None, d_total=p + 4400)
    for bad in (dict(stride=4095), dict(count=pkg.SR_MAX_SLOTS + 1), dict(d_total=None), dict(d_slots=None),
                dict(d_lens=None), dict(d_bytes=None), dict(stride=pkg.SR_MAX_SLOT_STRIDE + 1)):
        with pytest.raises(pkg.SrError) as e:
            router.frame_slots(**{**ok, **bad})
        assert e.value.errno == errno.EINVAL, bad
    assert pkg.lib().sr_frame_slots(router.handle, None) == -errno.EINVAL
    router.frame_slots(**ok)
    torch.cuda.synchronize()
    assert int(buf[4400:4408].cpu().numpy().view(np.uint64)[0]) == 0   # one empty datagram
