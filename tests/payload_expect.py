"""What sr_pack_payloads must write, from the oracle's descriptors, and a runner for the device chain
route -> pack -> payloads on poisoned buffers. A plain helper module (no fixtures): the expectation
functions need no GPU (tests/test_payload_abi.py uses them on the CPU)."""
from __future__ import annotations

import numpy as np

POISON = 0x5A
STRIDE = 1456


def as_u8(data):
    """bytes or an array as a contiguous np.uint8 array."""
    if isinstance(data, (bytes, bytearray)):
        return np.frombuffer(bytes(data), dtype=np.uint8)
    return np.ascontiguousarray(data, dtype=np.uint8)


def flat_expectation(data, sorted_recs, packets, pending):
    """The arena of a batch: per descriptor, in descriptor order, pending[shard][:carry] + its lines.
    Returns (arena bytes, offsets [n + 1], carry ranges [(lo, hi), ...])."""
    raw = bytes(data)
    parts, offs, rooms, at = [], [0], [], 0
    for p in packets:
        s, carry = int(p["shard"]), int(p["carry"])
        lead = bytes(pending.get(s, b""))[:carry]
        assert len(lead) == carry, (s, carry, len(lead))
        body = b"".join(raw[int(r["offset"]): int(r["offset"]) + int(r["length"])]
                        for r in sorted_recs[int(p["first"]): int(p["first"]) + int(p["nlines"])])
        assert len(body) == int(p["length"])
        if carry:
            rooms.append((at, at + carry))
        parts += [lead, body]
        at += carry + len(body)
        offs.append(at)
    return b"".join(parts), np.array(offs, dtype=np.uint32), rooms


def random_pending(rng, fills, avoid=None):
    """{shard: bytes} of the given lengths (no byte equal to `avoid`)."""
    out = {}
    for s, f in enumerate(fills):
        b = rng.integers(0, 256, int(f), dtype=np.uint8)
        if avoid is not None:
            b[b == avoid] = avoid ^ 1
        out[s] = b.tobytes()
    return out


def pending_image(pending, n, lengths=None, poison=POISON):
    """n pending slots of STRIDE bytes: slot s holds pending[s][:lengths[s]], poison elsewhere."""
    img = np.full(max(n, 1) * STRIDE, poison, dtype=np.uint8)
    for s in range(n):
        b = bytes(pending.get(s, b""))
        k = len(b) if lengths is None else int(lengths[s])
        assert k <= len(b) or lengths is None
        img[s * STRIDE: s * STRIDE + k] = np.frombuffer(b[:k], dtype=np.uint8)
    return img


class Expect:
    """The oracle's view of one batch: routing, packing, arena, offsets, pending after."""

    def __init__(self, oracle, data, n, alive, fills, pending):
        self.data = as_u8(data)
        self.n = n
        recs, _, self.n_lines = oracle.route(self.data, n, alive)
        self.probed = oracle.probed_dead(self.data, n, alive) if alive is not None else np.zeros(0, np.int64)
        self.sorted, self.packets, self.fill_out, self.n_valid = oracle.pack_packets(recs, n, fills, self.probed)
        self.pending = dict(pending)
        self.arena, self.offsets, self.rooms = flat_expectation(self.data, self.sorted, self.packets, self.pending)
        self.flushed, self.new_pending = oracle.materialize(self.data, self.sorted, self.packets, self.pending,
                                                            self.fill_out)
        assert [len(self.new_pending.get(s, b"")) for s in range(n)] == [int(f) for f in self.fill_out]

    @property
    def total(self):
        return int(self.offsets[-1])


class DeviceBatch:
    """Device buffers of one batch, every output prefilled with POISON."""

    def __init__(self, torch, pkg, data, n, fills, pending=None, *, max_records=None, max_packets=None,
                 payload_cap=None, lead=None, in_poison=b"\xEE", pend_out=True, slack=64):
        data = as_u8(data)
        self.nbytes = int(data.size)
        self.n = n
        if lead is None:
            self.d_in = torch.from_numpy(data.copy() if data.size else np.zeros(1, np.uint8)).cuda()
            self.in_ptr = self.d_in.data_ptr()
        else:   # the batch at an odd address between poison
            import byte_streams

            buf, off = byte_streams.embed(data, lead, in_poison)
            self.d_in = torch.from_numpy(buf.copy()).cuda()
            self.in_ptr = self.d_in.data_ptr() + off
        self.cap = max(self.nbytes, 1) if max_records is None else max_records   # never more lines than bytes
        self.mp = pkg.max_packets(self.nbytes, n) if max_packets is None else max_packets
        self.pcap = pkg.payload_capacity(self.nbytes, n) if payload_cap is None else payload_cap
        self.slack = slack
        z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device="cuda")
        self.d_rec, self.d_srt = z(self.cap, torch.int64), z(self.cap, torch.int64)
        self.d_cnt, self.d_counts = z(1, torch.int64), z(3, torch.int64)
        self.d_pd = z((n + 63) // 64, torch.int64)
        self.d_pk = z(2 * pkg.max_packets(self.nbytes, n), torch.int64)
        f = np.zeros(max(n, 1), dtype=np.uint16)
        if fills is not None:
            f[:n] = np.asarray(fills, dtype=np.uint16)
        self.d_fin = torch.from_numpy(f.view(np.int16).copy()).cuda()
        self.d_fout = z(n, torch.int16)
        self.d_pin = None if pending is None else torch.from_numpy(pending_image(pending, n)).cuda()
        self.d_pout = torch.full((max(n, 1) * STRIDE,), POISON, dtype=torch.uint8, device="cuda") \
            if (pend_out and pending is not None) else None
        self.d_arena = torch.full((self.pcap + slack,), POISON, dtype=torch.uint8, device="cuda")
        self.d_off = torch.full((4 * (self.mp + 1) + slack,), POISON, dtype=torch.uint8, device="cuda")
        self.d_total = torch.full((1,), -1, dtype=torch.int64, device="cuda")

    def route_pack_tuple(self):
        return (self.in_ptr, self.nbytes, self.d_rec.data_ptr(), self.cap, None, self.d_cnt.data_ptr(),
                self.d_pd.data_ptr(), self.d_fin.data_ptr(), self.d_srt.data_ptr(), self.d_pk.data_ptr(), self.mp,
                self.d_counts.data_ptr(), self.d_fout.data_ptr())

    def payload_tuple(self, pend_in="own", pend_out="own"):
        pin = (self.d_pin.data_ptr() if self.d_pin is not None else 0) if pend_in == "own" else pend_in
        pout = (self.d_pout.data_ptr() if self.d_pout is not None else 0) if pend_out == "own" else pend_out
        return (self.in_ptr, self.nbytes, self.d_srt.data_ptr(), self.cap, self.d_pk.data_ptr(), self.mp,
                self.d_counts.data_ptr(), self.d_fout.data_ptr(), pin, pout, self.d_arena.data_ptr(), self.pcap,
                self.d_off.data_ptr(), self.d_total.data_ptr())

    def refill(self):
        """Poison the outputs again (before another run into the same buffers)."""
        self.d_arena.fill_(POISON)
        self.d_off.fill_(POISON)
        self.d_total.fill_(-1)
        if self.d_pout is not None:
            self.d_pout.fill_(POISON)


def run(r, batches):
    """One sr_route_pack_many + one sr_pack_payloads_many over the batches (on the router's stream)."""
    r.route_pack_many([b.route_pack_tuple() for b in batches])
    r.pack_payloads_many([b.payload_tuple() for b in batches])


def check(b, e, *, room=False, label=""):
    """Every output buffer of DeviceBatch b, whole, against Expect e."""
    n_desc = min(len(e.packets), b.mp)
    counts = b.d_counts.cpu().tolist()
    assert counts == [len(e.packets), e.n_valid, e.n_lines], (label, counts)
    assert int(b.d_total.item()) == int(e.offsets[n_desc]), (label, int(b.d_total.item()), int(e.offsets[n_desc]))
    # offsets: [0, n + 1) written, the rest untouched
    want_off = np.full(b.d_off.numel(), POISON, dtype=np.uint8)
    want_off[: 4 * (n_desc + 1)] = e.offsets[: n_desc + 1].view(np.uint8)
    assert np.array_equal(b.d_off.cpu().numpy(), want_off), f"{label}: offsets differ"
    # arena: the descriptors' bytes below min(total, cap); the carries' room untouched in room mode
    want = np.full(b.pcap + b.slack, POISON, dtype=np.uint8)
    upto = min(int(e.offsets[n_desc]), b.pcap)
    flat = np.frombuffer(e.arena, dtype=np.uint8)
    want[:upto] = flat[:upto]
    if room:
        for lo, hi in e.rooms:
            want[min(lo, upto): min(hi, upto)] = POISON
    got = b.d_arena.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{label}: arena differs at {bad[:8].tolist()} ({bad.size} bytes) of {upto}")
    if b.d_pout is not None and n_desc == len(e.packets):
        want_p = pending_image(e.new_pending, b.n)
        got_p = b.d_pout.cpu().numpy()
        if not np.array_equal(got_p, want_p):
            bad = np.nonzero(got_p != want_p)[0]
            raise AssertionError(f"{label}: pending slots differ at {bad[:8].tolist()} "
                                 f"(slot {int(bad[0]) // STRIDE}, {bad.size} bytes)")
