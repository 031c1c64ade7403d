"""What the owner side of the regroup (sr_exchange_dead, sr_owner_pack, sr_flush_pending) must write,
from the oracle alone, and a runner for the multi-rank sequence with the ranks as threads of one process
on one GPU (the mailbox transport of tests/test_gpu_regroup.py, which also carries tag 2). A plain helper
module (no fixtures): the expectation functions need no GPU."""
from __future__ import annotations

import ctypes
import importlib
import threading
import traceback

import numpy as np

import payload_expect as X

POISON = X.POISON
STRIDE = X.STRIDE
LINE_LENS = [6, 64, 300, 1449]


def batch_bytes(pkg, seed, nbytes, tail=b""):
    """A framed batch of about nbytes (2-8 KiB in the tests): mixed line lengths, about 10 % invalid."""
    d = pkg.gen_stream(nbytes, LINE_LENS, seed=seed, p_invalid=0.1).data
    if tail:
        d = np.concatenate([d, np.frombuffer(pkg.frame_datagrams([tail]), dtype=np.uint8)])
    return np.ascontiguousarray(d)


def rank_alive(rank, world, n):
    """Alive snapshots that differ between the ranks. With several ranks: every rank has the shards rank 1
    owns dead, so rank 1 receives nothing at all (its pending bytes pass through, apart from the drop); the
    last of three or more ranks also has its own shards dead, so its own chunk is empty while rank 1, with
    a different snapshot, sends to those shards; a few more dead shards differ by rank."""
    alive = np.ones(n, dtype=np.int64)
    for k in range(n):
        if k % 7 == (3 + rank) % 7:
            alive[k] = 0
        if world > 1 and k % world == 1:
            alive[k] = 0
        if world > 2 and rank == world - 1 and k % world == rank:
            alive[k] = 0
    if world == 1 and n == 1:
        alive[:] = 1
    return alive.tolist()


def rank_inputs(pkg, oracle, rank, world, n, seed, nb=2, alive=None):
    """(datas, records, alive) of one rank's launch: two batches of 2-8 KiB. With several ranks, rank 0
    has no valid line (it sends nothing)."""
    alive = rank_alive(rank, world, n) if alive is None else alive
    datas = []
    for b in range(nb):
        if rank == 0 and world > 1:
            d = np.frombuffer(pkg.frame_datagrams([b"no colon here\n", b"x\n", b"AAAA" * 300]), dtype=np.uint8)
        else:
            d = batch_bytes(pkg, seed + 17 * rank + b, 2048 + 1531 * ((rank + 2 * b + seed) % 5),
                            (b"tail.%d.%d:1|c" % (rank, b)) + b"z" * ((rank + b) % 4))
        datas.append(np.ascontiguousarray(d))
    recs = [oracle.route(d, n, alive)[0] for d in datas]
    return datas, recs, alive


def expected_receive(oracle, inputs, world, r):
    """Owner r's receive buffer: every source's chunk r of its oracle pack, source by source, the records
    rebased into the concatenated bytes. Returns (bytes, records, counts [world, 2])."""
    packs = [oracle.pack_many_by_owner(d, rc, world) for d, rc, _ in inputs]
    eb = np.concatenate([pb[int(cnt[:r, 1].sum()):][: int(cnt[r, 1])] for pb, pr, cnt in packs])
    er, base = [], 0
    for pb, pr, cnt in packs:
        x = pr[int(cnt[:r, 0].sum()):][: int(cnt[r, 0])].copy()
        x["offset"] += np.uint32(base)
        er.append(x)
        base += int(cnt[r, 1])
    return np.asarray(eb, dtype=np.uint8), np.concatenate(er), np.stack([p[2][r] for p in packs])


def source_dead(oracle, inp, n):
    """The shards one source's launch probed dead: the OR over its batches (oracle.probed_dead)."""
    datas, _, alive = inp
    out = set()
    for d in datas:
        out |= {int(k) for k in oracle.probed_dead(d, n, alive)}
    return out


def dead_rows(oracle, inputs, n):
    """d_all_dead as every rank must hold it: u64 [world, nwords]."""
    nw = max((n + 63) // 64, 1)
    rows = np.zeros((len(inputs), nw), dtype=np.uint64)
    for p, inp in enumerate(inputs):
        for k in source_dead(oracle, inp, n):
            rows[p, k >> 6] |= np.uint64(1) << np.uint64(k & 63)
    return rows


class OwnerExpect:
    """One owner's outputs of one launch, in the issue's oracle terms: the drop first, then the stream."""

    def __init__(self, oracle, n, stream_bytes, stream_recs, dead, fills, pending):
        self.n = n
        self.bytes, self.recs = X.as_u8(stream_bytes), stream_recs
        self.dead = sorted(int(k) for k in dead)
        self.fill_eff = np.asarray(fills, dtype=np.uint16).copy()
        self.pending_eff = dict(pending)
        for s in self.dead:
            self.fill_eff[s] = 0
            self.pending_eff[s] = b""
        self.pending_eff = {s: bytes(self.pending_eff.get(s, b""))[: int(self.fill_eff[s])] for s in range(n)}
        self.sorted, self.packets, self.fill_out, self.n_valid = oracle.pack_packets(self.recs, n, self.fill_eff, ())
        self.n_lines = len(self.recs)
        self.arena, self.offsets, _ = X.flat_expectation(self.bytes, self.sorted, self.packets, self.pending_eff)
        self.flushed, self.new_pending = oracle.materialize(self.bytes, self.sorted, self.packets, self.pending_eff,
                                                            self.fill_out)
        assert [len(self.new_pending.get(s, b"")) for s in range(n)] == [int(f) for f in self.fill_out]

    @property
    def total(self):
        return int(self.offsets[-1])


class FlushExpect:
    """sr_flush_pending: one descriptor per non-empty slot in shard order, its bytes, the fills left."""

    def __init__(self, pkg, n, fills, pending, max_packets, payload_cap):
        shards = [s for s in range(n) if int(fills[s]) > 0]
        self.needed = len(shards)
        shards = shards[:max_packets]
        self.packets = np.zeros(len(shards), dtype=pkg.PACKET_DTYPE)
        self.packets["shard"] = shards
        self.packets["carry"] = [int(fills[s]) for s in shards]
        self.offsets = np.concatenate([[0], np.cumsum(self.packets["carry"].astype(np.int64))]).astype(np.uint32)
        self.arena = b"".join(bytes(pending[s])[: int(fills[s])] for s in shards)
        self.sent = {}
        self.fill_after = np.asarray(fills, dtype=np.uint16).copy()
        for i, s in enumerate(shards):
            if int(self.offsets[i + 1]) <= payload_cap:   # whole in the arena: flushed, its fill reset
                self.fill_after[s] = 0
                self.sent[s] = bytes(pending[s])[: int(fills[s])]

    @property
    def total(self):
        return int(self.offsets[-1])


def _whole(got, want, label):
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{label} differs at {bad[:8].tolist()} ({bad.size} of {got.size})")


def check_arena(op, packets, offsets, arena, needed, label):
    """The descriptor, offset, total and arena buffers of an OwnerPacker, whole, against the expectation
    (`needed` descriptors wanted, the first op.mp of them written; the arena cut at op.pcap)."""
    n_desc = min(len(packets), op.mp)
    got_pk = op.packets.cpu().numpy().view(np.uint8)
    want_pk = np.full(got_pk.size, POISON, dtype=np.uint8)
    want_pk[: 16 * n_desc] = np.ascontiguousarray(packets[:n_desc]).view(np.uint8)
    _whole(got_pk, want_pk, f"{label}: descriptors")
    assert int(op.counts[0].item()) == needed, (label, op.counts.cpu().tolist(), needed)
    assert int(op.total.item()) == int(offsets[n_desc]), (label, int(op.total.item()), int(offsets[n_desc]))
    want_off = np.full(op.offsets.numel(), POISON, dtype=np.uint8)
    want_off[: 4 * (n_desc + 1)] = np.ascontiguousarray(offsets[: n_desc + 1]).view(np.uint8)
    _whole(op.offsets.cpu().numpy(), want_off, f"{label}: offsets")
    want = np.full(op.pcap + op.slack, POISON, dtype=np.uint8)
    upto = min(int(offsets[n_desc]), op.pcap)
    want[:upto] = np.frombuffer(arena, dtype=np.uint8)[:upto]
    _whole(op.arena.cpu().numpy(), want, f"{label}: arena")


def check_owner(pkg, op, e, label=""):
    """Every output buffer of the OwnerPacker's last pack(), whole, against OwnerExpect e."""
    counts = op.counts.cpu().tolist()
    assert counts == [len(e.packets), e.n_valid, e.n_lines], (label, counts, len(e.packets), e.n_valid, e.n_lines)
    got_s = op.sorted.cpu().numpy().view(np.uint8)
    want_s = np.full(got_s.size, POISON, dtype=np.uint8)
    want_s[: 8 * e.n_lines] = np.ascontiguousarray(e.sorted).view(np.uint8)
    _whole(got_s, want_s, f"{label}: sorted records")
    check_arena(op, e.packets, e.offsets, e.arena, len(e.packets), label)
    got_f = op.fill[op.cur].cpu().numpy().view(np.uint16)[: e.n]
    assert np.array_equal(got_f, e.fill_out), (label, got_f.tolist(), e.fill_out.tolist())
    if min(len(e.packets), op.mp) == len(e.packets):
        _whole(op.pend[op.cur].cpu().numpy(), X.pending_image(e.new_pending, e.n), f"{label}: pending slots")


def check_flush(pkg, op, e, label=""):
    """Every output buffer of the OwnerPacker's last flush(), whole, against FlushExpect e."""
    assert op.counts.cpu().tolist() == [e.needed, 0, 0], (label, op.counts.cpu().tolist(), e.needed)
    check_arena(op, e.packets, e.offsets, e.arena, e.needed, label)
    got_f = op.fill[op.cur].cpu().numpy().view(np.uint16)[: len(e.fill_after)]
    assert np.array_equal(got_f, e.fill_after), (label, got_f.tolist(), e.fill_after.tolist())


def hip_runtime():
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip


D2H, H2D, D2D = 2, 1, 3


def mailbox_class(pkg, world):
    """The mailbox transport of test_gpu_regroup.py's multi-rank test (ranks are threads; a send copies the
    device bytes to a host blob in a shared box, the matching receive copies it back in at group_end),
    keyed by tag, so that the probed-dead rows (tag 2) travel like the lines (0) and records (1)."""
    hip = hip_runtime()
    box, cond, state = {}, threading.Condition(), {"abort": False}

    class Mailbox(pkg.Transport):
        def __init__(self, rank, router):
            self.rank, self.router, self.posted, self.step, self.calls = rank, router, [], 0, []

        def _put(self, key, blob):
            with cond:
                box.setdefault(key, []).append(blob)
                cond.notify_all()

        def _take(self, key):
            with cond:
                cond.wait_for(lambda: box.get(key) or state["abort"], timeout=60)
                assert box.get(key), ("nothing arrived (a peer failed?)", key)
                return box[key].pop(0)

        @staticmethod
        def abort():
            """A rank failed: its peers stop waiting for what it will never send."""
            with cond:
                state["abort"] = True
                cond.notify_all()

        def sizes(self, d_cnt, d_rcv):
            self.router.sync()
            sent = np.zeros((world, 2), np.uint64)
            assert hip.hipMemcpy(sent.ctypes.data, d_cnt, sent.nbytes, D2H) == 0
            for q in range(world):
                self._put(("sz", self.step, self.rank, q), sent[q].copy())
            received = np.stack([self._take(("sz", self.step, q, self.rank)) for q in range(world)])
            assert hip.hipMemcpy(d_rcv, received.ctypes.data, received.nbytes, H2D) == 0
            self.step += 1
            return sent, received

        def group_start(self):
            self.calls.append("group_start")
            self.router.sync()   # the kernels before the sends wrote what they read
            self.posted = []

        def send(self, addr, n, peer, tag):
            self.calls.append(("send", peer, tag, n))
            blob = ctypes.create_string_buffer(n)
            assert hip.hipMemcpy(ctypes.addressof(blob), addr, n, D2H) == 0
            self._put(("d", self.rank, peer, tag), blob)

        def recv(self, addr, n, peer, tag):
            self.calls.append(("recv", peer, tag, n))
            self.posted.append((addr, n, peer, tag))

        def group_end(self):
            self.calls.append("group_end")
            for addr, n, peer, tag in self.posted:
                blob = self._take(("d", peer, self.rank, tag))
                assert len(blob) == n and hip.hipMemcpy(addr, ctypes.addressof(blob), n, H2D) == 0

        def copy(self, dst, src, n):
            self.calls.append("copy")
            assert hip.hipMemcpy(dst, src, n, D2D) == 0

        def rebase(self, recs_addr, peers, n_lines):
            self.router.exchange_rebase(recs_addr, peers)
            self.router.sync()

    return Mailbox


def run_ranks(pkg, n, launches, fills, pendings, check, finish=None, packer=None, use_comm=False):
    """`world` ranks as threads on one GPU, each its own context and stream. launches[step][rank] =
    (datas, recs, alive); fills[rank] / pendings[rank]: the owner's pending state before the first launch.
    Per launch and rank: route with bitmaps, sr_regroup_run and sr_exchange_dead_run on the mailbox, then
    sr_owner_pack through an OwnerPacker with poisoned outputs; check(rank, step, op, received, rb, rr,
    mailbox) runs on the rank's thread after its stream has drained, finish(rank, op, router) after the last
    launch. packer: more OwnerPacker arguments (room). use_comm (one rank): sr_regroup_launch and
    sr_exchange_dead on a one-rank RCCL communicator instead of the mailbox. Returns {rank: mailbox calls}."""
    import torch

    rg = importlib.import_module("statsd-router_amd.regroup")
    world = len(launches[0])
    Mailbox = mailbox_class(pkg, world)
    errs, calls = {}, {}

    def rank_main(r):
        try:
            torch.cuda.set_device(0)
            nb = max(len(step[r][0]) for step in launches)
            cap = max(d.size for step in launches for d in step[r][0])
            total = max(sum(int(d.size) for d in step[r][0]) for step in launches)
            # (the exchange keeps every line 4-byte aligned: the received bytes can exceed the lines' own)
            recv_cap = pkg.pack_capacity(max(sum(int(d.size) for inp in step for d in inp[0]) for step in launches)) + 64
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
            d_in, d_rec, d_n = z((nb, cap), torch.uint8), z((nb, cap), torch.int64), z(nb, torch.int64)
            d_pd = z((nb, max((n + 63) // 64, 1)), torch.int64)
            pcap = pkg.pack_capacity(total)
            packed, precs = z(pcap, torch.uint8), z(nb * cap, torch.int64)
            counts, rcv = z((world, 2), torch.int64), z((world, 2), torch.int64)
            with pkg.Router(n, cap) as router:
                op = rg.OwnerPacker(pkg, router, world, recv_cap, recv_cap, poison=POISON, **(packer or {}))
                comm = pkg.Comm(pkg.Comm.new_id(), 1, 0, 0) if use_comm else None
                op.set_pending(fills[r], X.pending_image(pendings[r], n, fills[r]))
                t = Mailbox(r, router)
                for step, per_rank in enumerate(launches):
                    datas, _, alive = per_rank[r]
                    for b, d in enumerate(datas):
                        d_in[b, : d.size].copy_(torch.from_numpy(d.copy()))
                    rb = torch.full((recv_cap,), 0xCD, dtype=torch.uint8, device="cuda")
                    rr = torch.full((recv_cap,), -1, dtype=torch.int64, device="cuda")
                    torch.cuda.synchronize()
                    router.set_alive(alive)
                    batches = [(d_in[b].data_ptr(), int(d.size), d_rec[b].data_ptr(), cap, d_n[b].data_ptr(),
                                d_pd[b].data_ptr()) for b, d in enumerate(datas)]
                    router.route_device_many([(db, k, dr, mr, None, dn, dp) for db, k, dr, mr, dn, dp in batches])
                    if comm is not None:
                        fits, sent, received = router.regroup_launch(
                            comm, batches, counts.data_ptr(), rcv.data_ptr(), packed.data_ptr(), pcap,
                            precs.data_ptr(), rb.data_ptr(), rb.numel(), rr.data_ptr(), rr.numel())
                    else:
                        fits, sent, received = router.regroup_run(
                            t, world, r, batches, counts.data_ptr(), rcv.data_ptr(), packed.data_ptr(), pcap,
                            precs.data_ptr(), rb.data_ptr(), rb.numel(), rr.data_ptr(), rr.numel())
                    assert fits
                    op.exchange_dead(comm if comm is not None else t, r, batches)
                    op.pack(rb.data_ptr(), int(received[:, 1].sum()), rr.data_ptr(), rcv.data_ptr())
                    router.sync()
                    check(r, step, op, received, rb, rr, t)
                if finish is not None:
                    finish(r, op, router)
                router.sync()
                if comm is not None:
                    comm.close()
                calls[r] = t.calls
        except Exception:   # noqa: BLE001
            errs[r] = traceback.format_exc()
            Mailbox.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not any(t.is_alive() for t in th), "a rank did not finish"
    assert not errs, "\n".join(f"rank {r}:\n{e}" for r, e in errs.items())
    return calls
