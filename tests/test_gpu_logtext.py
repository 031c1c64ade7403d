"""GPU: sr_format_log, a routed batch's log text written on the device, byte for byte against
tests/log_expect.py (pinned to the reference by tests/test_log_expect.py). The records and hashes come from
the CPU oracle, so the test drives the formatter alone. Every output (text, offsets, levels, total, message
count) is prefilled with a poison byte, lies between 64 guard bytes and is compared whole, so a byte written
where none belongs (past the total, past the capacity, into a neighbour's piece, past the index) fails the
test as surely as a wrong one."""
from __future__ import annotations

import errno
import functools

import numpy as np
import pytest

import byte_streams as B
import log_expect as L

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = 0xCD
RECS = 128          # records per workgroup of log_lens_kernel / log_write_kernel (kLogRecs)
RECORD = np.dtype([("offset", "<u4"), ("length", "<u2"), ("route", "<u2")])


@pytest.fixture(scope="module")
def routers(pkg):
    """Contexts by n_downstreams, opened on first use."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = pkg.Router(n, 1 << 20)
        return made[n]

    yield get
    for r in made.values():
        r.close()


def _dev(torch, arr, mis=0, tail=0):
    """(tensor, address): the array's bytes `mis` bytes past an allocation's start, poison around them."""
    raw = np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint8)
    t = torch.full((mis + raw.size + tail,), POISON, dtype=torch.uint8, device="cuda")
    if raw.size:
        t[mis: mis + raw.size].copy_(torch.from_numpy(raw.copy()))
    return t, t.data_ptr() + mis


def _out(torch, nbytes, mis=0):
    t = torch.full((GUARD + mis + nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + GUARD + mis


class Log:
    """One sr_format_log call on device buffers and the comparison of everything it may have written."""

    def __init__(self, torch, data, recs, hashes, ends, n, *, min_level=0, prefixes=(b"", b""), max_msg=0,
                 text_cap=None, max_msgs=None, max_records=None, src_mis=0, dst_mis=0, pfx_mis=0, index=True,
                 slack=0):
        self.torch = torch
        data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, dtype=np.uint8)
        recs = np.ascontiguousarray(recs, dtype=RECORD)
        self.want = L.expect(data, recs, hashes, ends, n, min_level, prefixes, max_msg, max_records)
        text, offs, lv = self.want
        self.cap = len(text) + slack if text_cap is None else text_cap
        self.max_msgs = lv.size + slack if max_msgs is None else max_msgs
        self.dst_mis, self.index = dst_mis, index
        self.keep = []
        self.d_bytes = self._in(data, src_mis)
        self.d_recs = self._in(recs)
        self.d_n = self._in(np.asarray([len(recs)], dtype=np.uint64))
        self.d_hashes = self._in(np.asarray(hashes, dtype=np.uint64)) if hashes is not None else None
        self.d_ends = self._in(np.asarray(ends, dtype=np.uint32)) if ends is not None and len(ends) else None
        self.d_prefix = self._in(np.frombuffer(prefixes[0] + prefixes[1], dtype=np.uint8), pfx_mis) if prefixes[0] + prefixes[1] else None
        self.args = dict(d_bytes=self.d_bytes if data.size else None, nbytes=int(data.size), d_recs=self.d_recs if len(recs) else None,
                         d_n_records=self.d_n, max_records=len(recs) if max_records is None else max_records,
                         d_hashes=self.d_hashes, d_ends=self.d_ends, n_datagrams=0 if self.d_ends is None else len(ends),
                         min_level=min_level, d_prefix=self.d_prefix, prefix_len=(len(prefixes[0]), len(prefixes[1])),
                         max_msg=max_msg, text_cap=self.cap, max_msgs=self.max_msgs)
        self.text, p_text = _out(torch, self.cap, dst_mis)
        self.offsets, p_off = _out(torch, 4 * (self.max_msgs + 1))
        self.levels, p_lv = _out(torch, self.max_msgs)
        self.total, p_total = _out(torch, 8)
        self.n_msgs, p_n = _out(torch, 8)
        self.args.update(d_text=p_text if self.cap else None, d_offsets=p_off if index else None,
                         d_levels=p_lv if index else None, d_total=p_total, d_n_msgs=p_n)

    def _in(self, arr, mis=0):
        t, p = _dev(self.torch, arr, mis)
        self.keep.append(t)
        return p

    def poison(self):
        for t in (self.text, self.offsets, self.levels, self.total, self.n_msgs):
            t.fill_(POISON)

    def run(self, r):
        r.format_log(**self.args)

    def _whole(self, t, at, body, label):
        want = np.full(t.numel(), POISON, dtype=np.uint8)
        want[at: at + body.size] = body
        got = t.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{label}: differs at {bad[:8].tolist()} of {want.size} (body at {at}, {body.size} bytes): "
                                 f"got {got[bad[:8]].tolist()} want {want[bad[:8]].tolist()}")

    def check(self, label="", want=None):
        text, offs, lv = self.want if want is None else want
        self.torch.cuda.synchronize()
        u8 = lambda a: np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)
        self._whole(self.total, GUARD, u8(np.asarray([len(text)], dtype="<u8")), f"{label}: total")
        self._whole(self.n_msgs, GUARD, u8(np.asarray([lv.size], dtype="<u8")), f"{label}: n_msgs")
        w = min(len(text), self.cap)
        self._whole(self.text, GUARD + self.dst_mis, np.frombuffer(text[:w], dtype=np.uint8), f"{label}: text")
        k = min(lv.size, self.max_msgs) if self.index else 0
        self._whole(self.offsets, GUARD, u8(offs[: k + 1].astype("<u4")) if self.index else np.zeros(0, np.uint8),
                    f"{label}: offsets")
        self._whole(self.levels, GUARD, lv[:k], f"{label}: levels")


@functools.lru_cache(maxsize=None)
def _ragged(seed):
    return B.ragged_stream(seed, B.RAGGED_MIN_BYTES)


def _route(oracle, data, n, alive=None):
    recs, hs, cnt = oracle.route(data, n, alive)
    return recs[:cnt].copy(), hs[:cnt].copy()


def _ends(oracle, dgrams):
    framed = [oracle.frame(d) for d in dgrams]
    return b"".join(framed), np.cumsum([len(f) for f in framed]).astype(np.uint32)


def _go(torch, r, label, *a, **k):
    log = Log(torch, *a, **k)
    log.run(r)
    log.check(label)
    return log


PFX = (b"2026-01-01 00:00:00 [TRACE] th0 ", b"W:")   # 32 and 2 bytes


# ---- 1. message kinds and numbers ---------------------------------------------------------------------------------
def test_every_message_kind(pkg, oracle, routers, torch_stream):
    import torch

    r = routers(4)
    r.set_stream(torch_stream.cuda_stream)
    dgrams = [b"a.b.c:1|c\nnocolon-here\n", b"x\n", b"::1|cc\n" + b"\xff\xfe:1|c", b"", b"y" * 1500, b"12345\n123456:\n"]
    data, ends = _ends(oracle, dgrams)
    for alive in (None, [1, 0, 1, 0], [0, 0, 0, 0]):
        recs, hs = _route(oracle, data, 4, alive)
        if alive is None:
            assert int(hs[recs["offset"].tolist().index(data.index(b"::1|cc"))]) == 0          # hash 0
            assert any(int(h) >> 63 for h in hs)                                               # top bit set
        for level in (0, 3):
            for pf in ((b"", b""), PFX):
                _go(torch, r, f"alive={alive} level={level}", data, recs, hs if level == 0 else None, ends, 4,
                    min_level=level, prefixes=pf)


def test_line_lengths_and_shard_ids(pkg, oracle, routers, torch_stream):
    """Lines of 6 and 1449 bytes, invalid lengths 1, 5, 1450 and 4096, shard ids of every digit count
    (synthetic routes: the formatter prints what the record says)."""
    import torch

    r = routers(pkg.SR_MAX_DOWNSTREAMS)
    r.set_stream(torch_stream.cuda_stream)
    lines = [b"a:1|c\n", b"n" * 1441 + b":1234|c\n", b"\n", b"abcd\n", b"L" * 1449 + b"\n", b"M" * 4095 + b"\n"]
    assert [len(x) for x in lines] == [6, 1449, 1, 5, 1450, 4096]
    data = b"".join(lines + [b"s%d:1|c\n" % i for i in range(6)])
    recs, hs = _route(oracle, data, pkg.SR_MAX_DOWNSTREAMS)
    assert recs["route"][2:6].tolist() == [0xFFFD] * 4 and recs["length"][5] == 4096
    recs["route"][6:12] = [0, 9, 10, 99, 100, 65532]
    ends = np.asarray([len(data)], dtype=np.uint32)
    _go(torch, r, "lengths and shards", data, recs, hs, None, pkg.SR_MAX_DOWNSTREAMS, prefixes=PFX)
    _go(torch, r, "one datagram", data, recs, hs, ends, pkg.SR_MAX_DOWNSTREAMS)


def test_no_downstreams(pkg, oracle, routers, torch_stream):
    import torch

    r = routers(0)
    r.set_stream(torch_stream.cuda_stream)
    data, ends = _ends(oracle, [b"a:1|c\nbb:2|c", b"nocolon\n"])
    recs, hs = _route(oracle, data, 0)
    assert recs["route"].tolist() == [0xFFFF, 0xFFFF, 0xFFFE]
    for level in (0, 3):
        _go(torch, r, f"n=0 level={level}", data, recs, hs, ends, 0, min_level=level, prefixes=PFX)


# ---- 2. NUL bytes ------------------------------------------------------------------------------------------------
def test_nul_bytes_cut_spans(pkg, oracle, routers, torch_stream):
    import torch

    r = routers(4)
    r.set_stream(torch_stream.cuda_stream)
    dgrams = [b"\0first:1|c\n", b"last:1|c\0\n", b"na\0me:1|c\n", b"\0\0\0\0\0\0\0\n", b"\0\n",
              b"ok:1|c\ncut\0here:1|c\nafter:2|c\n",        # the NUL cuts "got packet" in its second line
              bytes(range(0x80, 0x100)) + b":1|c\n", b"\0nocolon\n", b"nocol\0on\n", b"z" * 1460 + b"\0" + b"z" * 20]
    data, ends = _ends(oracle, dgrams)
    recs, hs = _route(oracle, data, 4)
    for level in (0, 3):
        _go(torch, r, f"NULs level={level}", data, recs, hs, ends, 4, min_level=level, prefixes=PFX)


@pytest.mark.parametrize("dst_mis", [0, 9])
def test_nul_at_piece_boundaries(pkg, oracle, routers, torch_stream, dst_mis):
    """One NUL at each position of a line around the 16-byte boundaries of the source loads and of the
    destination pieces, one byte either side included."""
    import torch

    r = routers(4)
    r.set_stream(torch_stream.cuda_stream)
    for src_mis in (0, 1, 15):
        lines = []
        for p in list(range(0, 40)) + [47, 48, 49, 63, 64, 65]:
            line = bytearray(b"m" * 70 + b":1|c\n")
            line[p] = 0
            lines.append(bytes(line))
        data, ends = _ends(oracle, lines)
        recs, hs = _route(oracle, data, 4)
        _go(torch, r, f"src+{src_mis}", data, recs, hs, ends, 4, src_mis=src_mis, dst_mis=dst_mis, prefixes=(b"", b"w"))


# ---- 3. alignment and prefixes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("a", range(16))
def test_alignments(pkg, oracle, routers, torch_stream, a):
    """d_bytes, d_text and the prefixes each at every one of the 16 byte alignments (the three move at
    different strides, so every call has them apart)."""
    import torch

    r = routers(4)
    r.set_stream(torch_stream.cuda_stream)
    rng = np.random.default_rng(a)
    data = B.cut_at_newline(_ragged(3), 0, 12000)
    recs, hs = _route(oracle, data, 4, [1, 1, 0, 1])
    cuts = np.flatnonzero(data == 10) + 1
    ends = np.unique(np.concatenate([cuts[rng.random(cuts.size) < 0.2], [data.size]])).astype(np.uint32)
    _go(torch, r, f"align {a}", data, recs, hs, ends, 4, src_mis=a, dst_mis=(7 * a + 3) % 16, pfx_mis=(11 * a + 5) % 16,
        prefixes=PFX)


@pytest.mark.parametrize("tlen,wlen", [(0, 1), (1, 0), (15, 16), (16, 17), (17, 35), (35, 15), (256, 255)])
def test_prefix_lengths(pkg, oracle, routers, torch_stream, tlen, wlen):
    import torch

    r = routers(4)
    r.set_stream(torch_stream.cuda_stream)
    data, ends = _ends(oracle, [b"a.b:1|c\nnocolon-line\nq\n", b"cc:2|c\n" * 9, b"\n" * 5])
    recs, hs = _route(oracle, data, 4, [1, 0, 0, 1])
    pf = (bytes(0x41 + i % 26 for i in range(tlen)), bytes(0x61 + i % 26 for i in range(wlen)))
    for level in (0, 3):
        _go(torch, r, f"prefix {tlen}/{wlen} level={level}", data, recs, hs, ends, 4, min_level=level, prefixes=pf,
            pfx_mis=3)


# ---- 4. max_msg ------------------------------------------------------------------------------------------------
def test_max_msg_cuts(pkg, oracle, routers, torch_stream):
    import torch

    r = routers(4)
    r.set_stream(torch_stream.cuda_stream)
    # 2047 against a 4095-byte datagram (one valid and one invalid line in it) and a 4096-byte invalid line
    d1 = b"v" * 1400 + b":1|c\n" + b"i" * 2689 + b"\n"
    assert len(d1) == 4095
    data, ends = _ends(oracle, [d1, b"J" * 4095, b"ok:1|c\n"])
    recs, hs = _route(oracle, data, 4)
    assert recs["length"].tolist() == [1405, 2690, 4096, 7]
    for mm in (0, 2047):
        _go(torch, r, f"max_msg {mm}", data, recs, hs, ends, 4, prefixes=PFX, max_msg=mm)
    # cuts inside the prefix's last byte + 1, inside the constant text, inside the hash, the length, the shard id
    data, ends = _ends(oracle, [b"\xf1name:1|c\nnocolon-line\nq\n", b"cc:2|c\n"])
    recs, hs = _route(oracle, data, 4)
    assert int(hs[0]) >> 60
    for mm in (33, 40, 32 + 24 + 7, 32 + 24 + 16 + 11, 32 + 39, 32 + 24, 32 + 24 + 16 + 11 + 1 + 9 + 3):
        _go(torch, r, f"max_msg {mm}", data, recs, hs, ends, 4, prefixes=PFX, max_msg=mm)
        _go(torch, r, f"max_msg {mm} WARN", data, recs, None, ends, 4, prefixes=PFX, max_msg=mm, min_level=3)
    # a value that does not clear both prefixes is refused
    for mm in (1, 2, 31, 32):
        log = Log(torch, data, recs, hs, ends, 4, prefixes=PFX, max_msg=mm)
        with pytest.raises(pkg.SrError) as e:
            log.run(r)
        assert e.value.errno == errno.EINVAL
        torch.cuda.synchronize()
        assert bool((log.text == POISON).all()) and bool((log.total == POISON).all())


# ---- 5. capacity ------------------------------------------------------------------------------------------------
def test_capacity_cuts(pkg, oracle, routers, torch_stream):
    """text_cap = total, total - 1, 0 and the middle of a message; max_msgs one short; max_records below the
    line count: nothing past the room is written and the totals still say the need."""
    import torch

    r = routers(4)
    r.set_stream(torch_stream.cuda_stream)
    data = B.cut_at_newline(_ragged(5), 0, 120000)
    recs, hs = _route(oracle, data, 4, [0, 1, 1, 1])
    ends = np.asarray([data.size], dtype=np.uint32)
    text, offs, lv = L.expect(data, recs, hs, ends, 4, 0, PFX)
    assert len(recs) > 2 * RECS and lv.size > RECS + 1
    mid = int(offs[lv.size // 2]) + 5
    for dst_mis in (0, 5):
        for cap in (len(text), len(text) - 1, 0, mid, int(offs[RECS]) + 1):
            _go(torch, r, f"cap {cap} dst+{dst_mis}", data, recs, hs, ends, 4, prefixes=PFX, text_cap=cap, dst_mis=dst_mis)
    for mm in (lv.size - 1, 1, 0, RECS):
        _go(torch, r, f"max_msgs {mm}", data, recs, hs, ends, 4, prefixes=PFX, max_msgs=mm)
    _go(torch, r, "no index", data, recs, hs, ends, 4, prefixes=PFX, index=False)
    for mr in (len(recs) - 1, RECS, 1, 0):
        _go(torch, r, f"max_records {mr}", data, recs, hs, ends, 4, prefixes=PFX, max_records=mr, slack=3)


# ---- 6. datagram ends -------------------------------------------------------------------------------------------
def test_datagram_ends(pkg, oracle, routers, torch_stream):
    import torch

    r = routers(4)
    r.set_stream(torch_stream.cuda_stream)
    dgrams = [b"a:1|c", b"", b"", b"bb:2|c\ncc:3|c\n", b"\n", b"", b"dd:4|c\nnocolon\n", b""]
    data, ends = _ends(oracle, dgrams)
    recs, hs = _route(oracle, data, 4)
    assert len(set(ends.tolist())) < len(ends)   # empty datagrams repeat an end
    got = _go(torch, r, "repeats", data, recs, hs, ends, 4, prefixes=PFX)
    assert got.want[0].count(b"got packet") == 4
    _go(torch, r, "NULL ends", data, recs, hs, None, 4, prefixes=PFX)
    for k in (1, 3, 4):
        _go(torch, r, f"ends stop after {k}", data, recs, hs, ends[:k], 4, prefixes=PFX)
    _go(torch, r, "WARN ignores ends", data, recs, None, ends, 4, prefixes=PFX, min_level=3)


# ---- 7. counts and extremes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 64, 65, RECS - 1, RECS, RECS + 1, 2 * RECS - 1, 2 * RECS, 2 * RECS + 1, 1024 * RECS + 5])
def test_record_counts_around_the_workgroup(pkg, oracle, routers, torch_stream, count):
    """One below, at and one above the writer's records per workgroup (its LDS tables hold one workgroup's
    messages, so that constant is its only chunk) and the scan's 1024-workgroup round."""
    import torch

    r = routers(4)
    r.set_stream(torch_stream.cuda_stream)
    kinds = [b"ab:1|c\n", b"\n", b"nocolon\n", b"m.n.o:22|g\n"]
    big = count > 10 * RECS
    data = b"".join(kinds[i % 4] if not big else b"\n" for i in range(count))
    recs, hs = _route(oracle, data, 4, [1, 1, 1, 0])
    assert len(recs) == count
    ends = np.asarray([len(data)] if big else np.cumsum([len(kinds[i % 4]) for i in range(count)])[2::3].tolist() + [len(data)], dtype=np.uint32)
    ends = np.unique(ends)
    _go(torch, r, f"count {count}", data, recs, hs, ends, 4, prefixes=PFX if not big else (b"", b"w"), dst_mis=count % 16)


def test_5000_one_byte_lines_within_the_macros(pkg, oracle, routers, torch_stream):
    import torch

    r = routers(4)
    r.set_stream(torch_stream.cuda_stream)
    data = b"\n" * 5000
    recs, hs = _route(oracle, data, 4)
    ends = np.arange(1, 5001, dtype=np.uint32)
    log = _go(torch, r, "5000", data, recs, hs, ends, 4, prefixes=PFX,
              text_cap=pkg.log_text_capacity(5000, 5000, 32), max_msgs=pkg.log_max_msgs(5000, 5000))
    assert log.want[2].size == 10000


def test_single_message_and_empty_batch(pkg, oracle, routers, torch_stream):
    import torch

    r = routers(4)
    r.set_stream(torch_stream.cuda_stream)
    data = b"\n"
    recs, hs = _route(oracle, data, 4)
    log = _go(torch, r, "one message", data, recs, None, None, 4, min_level=3, slack=20)
    assert log.want[0] == b"udp_read_cb: invalid length 1 of metric \n\n"
    empty = np.zeros(0, dtype=RECORD)
    _go(torch, r, "nbytes 0", b"", empty, None, None, 4, slack=20)
    _go(torch, r, "nbytes 0 TRACE", b"", empty, np.zeros(0, np.uint64), np.zeros(0, np.uint32), 4, slack=20, prefixes=PFX)
    # a routed batch none of whose lines has a message at WARN
    data = b"ab:1|c\ncd:2|c\n"
    recs, hs = _route(oracle, data, 4)
    log = _go(torch, r, "no WARN", data, recs, None, None, 4, min_level=3, slack=20)
    assert log.want[2].size == 0


# ---- 8. random streams ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ragged_streams(pkg, oracle, routers, torch_stream, seed):
    import torch

    r = routers(7)
    r.set_stream(torch_stream.cuda_stream)
    rng = np.random.default_rng(seed)
    data = B.cut_at_newline(_ragged(seed), 0, 200000)
    cuts = np.flatnonzero(data == 10) + 1
    ends = np.unique(np.concatenate([cuts[rng.random(cuts.size) < 0.1], [data.size]])).astype(np.uint32)
    for alive in (None, (rng.random(7) < 0.5).astype(int).tolist(), [0] * 7):
        recs, hs = _route(oracle, data, 7, alive)
        for level, mm in ((0, 0), (0, 2047), (3, 0)):
            _go(torch, r, f"seed {seed} alive={alive} level={level} max_msg={mm}", data, recs, hs, ends, 7,
                min_level=level, prefixes=PFX, max_msg=mm, src_mis=seed, dst_mis=3 * seed)


# ---- 9. graph capture ------------------------------------------------------------------------------------------
def test_captured_call_replays_on_changed_inputs(pkg, oracle, routers, torch_stream):
    import torch

    r = routers(4)
    r.set_stream(torch_stream.cuda_stream)
    batches = []
    for k, alive in ((0, None), (1, [1, 0, 0, 1]), (2, [0, 0, 0, 0])):
        dg = [b"k%d.%d:1|c\n" % (k, i) * (1 + (i + k) % 5) + (b"bad\0line\n" if i % 3 == k else b"") for i in range(300)]
        data, ends = _ends(oracle, dg)
        recs, hs = _route(oracle, data, 4, alive)
        batches.append((data, recs, hs, ends))
    room = max(len(b[0]) for b in batches) + 64
    nrec = max(len(b[1]) for b in batches) + 5
    # fixed-size inputs, so that one captured call serves every batch
    def padded(b):
        data, recs, hs, ends = b
        return (np.frombuffer(data.ljust(room, b"\n"), dtype=np.uint8), np.concatenate([recs, np.zeros(nrec - len(recs), RECORD)]),
                np.concatenate([hs, np.zeros(nrec - len(hs), np.uint64)]), np.concatenate([ends, np.full(300 - len(ends), ends[-1], np.uint32)]))

    d0, r0, h0, e0 = padded(batches[0])
    cap = max(len(L.expect(*b, 4, 0, PFX)[0]) for b in batches) + 100
    log = Log(torch, d0, r0, h0, e0, 4, prefixes=PFX, text_cap=cap, max_msgs=3 * nrec)
    log.keep[2].copy_(torch.from_numpy(np.frombuffer(np.uint64(len(batches[0][1])).tobytes(), dtype=np.uint8).copy()))
    log.run(r)   # eager: the context's scan scratch is allocated outside the capture
    log.check("eager", want=L.expect(*batches[0], 4, 0, PFX))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch_stream):
        log.run(r)
    for label, b in (("replay 1", batches[1]), ("replay 2", batches[2]), ("replay 3", batches[0])):
        d, rr, h, e = padded(b)
        for t, arr in zip(log.keep[:5], (d, rr, np.asarray([len(b[1])], np.uint64), h, e)):
            t.copy_(torch.from_numpy(np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint8).copy()))
        log.poison()
        g.replay()
        log.check(label, want=L.expect(*b, 4, 0, PFX))


# ---- 10. argument errors on a live context ---------------------------------------------------------------------
def test_argument_errors(pkg, oracle, routers, torch_stream):
    import torch

    r = routers(4)
    r.set_stream(torch_stream.cuda_stream)
    data = b"a:1|c\nnocolon\n"
    recs, hs = _route(oracle, data, 4)
    log = Log(torch, data, recs, hs, np.asarray([len(data)], np.uint32), 4, prefixes=PFX)
    ok = dict(log.args)
    for bad in (dict(d_total=None), dict(d_n_msgs=None), dict(d_n_records=None), dict(d_bytes=None), dict(d_recs=None),
                dict(d_hashes=None), dict(d_prefix=None), dict(d_text=None), dict(min_level=-1), dict(min_level=4),
                dict(nbytes=(1 << 20) + 1), dict(prefix_len=(257, 2)), dict(prefix_len=(32, 257)), dict(max_msg=32)):
        with pytest.raises(pkg.SrError) as e:
            r.format_log(**{**ok, **bad})
        assert e.value.errno == errno.EINVAL, bad
    assert pkg.lib().sr_format_log(r.handle, None) == -errno.EINVAL
    torch.cuda.synchronize()
    assert bool((log.text == POISON).all())
    r.format_log(**{**ok, "d_hashes": None, "min_level": 3})   # no hashes needed at WARN
    log.check("WARN without hashes", want=L.expect(data, recs, None, None, 4, 3, PFX))
