"""GPU: sr_validate, the line grammar on the device, against tests/validate_expect.py. Records and hashes come from
the restatement's own tokeniser or are made up, so the stage is driven alone. Every buffer lies between guard bytes
and is compared whole: the records out, the hashes out, the reasons and the room behind them, the four counts, and
the inputs, which must come back unchanged. The hits are compared exactly."""
from __future__ import annotations

import errno

import numpy as np
import pytest

import validate_expect as E
from test_gpu_coalesce import Buf

pytestmark = pytest.mark.gpu

INTERESTING = bytes([0, 1, 9, 10, 13, 32, 33, 34, 35, 43, 44, 49, 100, 104, 45, 46, 47, 48, 57, 58, 64, 99, 103, 109, 115, 124, 126, 127, 128, 255])


def made_up(lines, n, seed=1):
    """The lines laid end to end exactly as given (a '\\n' only where the line has one) and a record per line."""
    data = b"".join(lines)
    recs = np.zeros(len(lines), E.RECORD_DTYPE)
    lens = np.array([len(x) for x in lines], np.int64)
    recs["offset"] = np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(lines) else []
    recs["length"] = lens
    recs["route"] = np.arange(len(lines)) % n
    hashes = np.random.default_rng(seed).integers(0, 1 << 62, len(lines)).astype(np.uint64)
    return data, recs, hashes


class DevBatch:
    def __init__(self, torch, spec, mis=(0, 0, 0), hashes=True, reason=True):
        self.data, self.recs = bytes(spec["data"]), np.ascontiguousarray(spec["recs"], E.RECORD_DTYPE)
        self.hashes = np.ascontiguousarray(spec["hashes"], np.uint64)
        self.n_records = len(self.recs) if spec.get("n_records") is None else spec["n_records"]
        self.max_records = len(self.recs) if spec.get("max_records") is None else spec["max_records"]
        self.with_hashes, self.with_reason = hashes, reason
        mb, mr, m8 = mis
        self.bytes = Buf(torch, self.data, None, mb)
        self.d_recs = Buf(torch, self.recs.tobytes(), None, mr)
        self.d_hashes = Buf(torch, self.hashes.tobytes() if len(self.hashes) else bytes(8), None, m8)
        self.d_n = Buf(torch, np.asarray([self.n_records], np.uint64).tobytes(), None, m8)
        self.out = Buf(torch, b"", 8 * self.max_records, mr)
        self.hout = Buf(torch, b"", 8 * self.max_records, m8)
        self.reason = Buf(torch, b"", self.max_records, mb & 3)
        self.counts = Buf(torch, b"", 32, m8)

    def tuple(self):
        mr = self.max_records
        return (self.bytes.ptr if self.bytes.size else 0, len(self.data), self.d_recs.ptr if mr else 0, self.d_n.ptr, mr,
                self.out.ptr if mr else 0, self.d_hashes.ptr if self.with_hashes else 0,
                self.hout.ptr if self.with_hashes else 0, self.reason.ptr if self.with_reason else 0, self.counts.ptr)

    def check(self, n, drop_mask, types, label):
        res = E.apply(self.data, self.recs, self.hashes, n, drop_mask, types, self.n_records, self.max_records)
        self.counts.expect(res.counts.tobytes(), f"{label}: counts")
        self.reason.expect(res.reason.tobytes() if self.with_reason else b"", f"{label}: reasons")
        self.out.expect(res.out.tobytes(), f"{label}: records out")
        self.hout.expect(res.hashes_out.tobytes() if self.with_hashes else b"", f"{label}: hashes out")
        self.bytes.expect(self.data, f"{label}: batch")
        self.d_recs.expect(self.recs.tobytes(), f"{label}: input records")
        self.d_hashes.expect(self.hashes.tobytes() if len(self.hashes) else bytes(8), f"{label}: hashes")
        self.d_n.expect(np.asarray([self.n_records], np.uint64).tobytes(), f"{label}: record count")
        return res


class Dev:
    """A context with the stage open on the test's stream."""

    def __init__(self, pkg, torch, stream, n, drop_mask=E.DROP_ALL, types=E.TYPES_ALL, max_batch=1 << 20):
        self.pkg, self.torch, self.n, self.drop_mask, self.types = pkg, torch, n, drop_mask, types
        self.r = pkg.Router(n, max_batch)
        self.r.set_stream(stream.cuda_stream)
        self.r.validate_open(pkg.ValidateConfig(drop_mask, types))
        self.hits = np.zeros((E.REASONS, 2), np.uint64)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.torch.cuda.synchronize()
        self.r.close()

    def upload(self, specs, **kw):
        return [DevBatch(self.torch, dict(zip(("data", "recs", "hashes"), s)) if isinstance(s, tuple) else s, **kw)
                for s in specs]

    def check(self, batches, label, calls=1):
        self.torch.cuda.synchronize()
        res = [b.check(self.n, self.drop_mask, self.types, f"{label}[{j}]") for j, b in enumerate(batches)]
        for x in res:
            self.hits += x.hits * np.uint64(calls)
        got = self.r.validate_read()
        assert got.tolist() == self.hits.tolist(), f"{label}: hits"
        return res

    def run(self, specs, label, **kw):
        batches = self.upload(specs, **kw)
        self.r.validate([b.tuple() for b in batches])
        return self.check(batches, label)


POOL = [b"svc.req:1|c", b"svc.t:12.5|ms|@0.25", b"a.b:-3|c|@1|#env:prod,z:a", b"g.x:+17|g|#t", b"u:alice:bob|s", b"lat:7|h|@0.1",
        b"dist:7|d", b"no colon here", b":1|c", b"a b:1|c", b"a:1", b"a:1|q", b"a:x|c", b"a:1|c|x", b"a:1|g|@1", b"a:1|c|#",
        b"a:1|c|#t|@1", b"a:" + b"1" * 21 + b"|c", b"ab", b"a:1|c|#" + b"t" * 90, b"n" * 70 + b":1|c"]


def mix(seed, count, n):
    """`count` lines of every reason, tokenised as the route launch would (unrouted lines are not subject)."""
    rng = np.random.default_rng(seed)
    return E.records_of([POOL[k] for k in rng.integers(0, len(POOL), count)], n)


def test_the_mutation_corpus_as_one_batch(pkg, torch_stream):
    """Every truncation of the seed lines and, at every position, two dozen byte values: NUL, '\\n', high bytes,
    the separators and the signs, in the name, the value, the type, the rate and the tags. About 8k lines."""
    import torch

    lines = []
    for ln in E.SEED_LINES:
        lines += [ln[:k] for k in range(1, len(ln) + 1)]
        lines += [ln[:at] + bytes([v]) + ln[at + 1:] for at in range(len(ln)) for v in INTERESTING if v != ln[at]]
    assert 7000 < len(lines) < 10000
    with Dev(pkg, torch, torch_stream, 3) as d:
        res, = d.run([made_up(lines, 3)], "mutations", mis=(5, 0, 0))
        assert (res.hits[:, 0] > 0).all() and int(res.counts[3]) == len(lines)


def test_every_start_alignment_and_the_separators_around_a_block_edge(pkg, torch_stream):
    """Names of 1..40 bytes, values of 1, 2 and 17 digits, with and without a rate and tags, behind fillers of 0..15
    bytes, in batches whose own address is moved by 0, 1, 7 and 15 bytes (so the first and the last 16-byte block
    are partial). The last line has no '\\n' and ends with the batch."""
    import torch

    lines = []
    for nl in range(1, 41):
        for k, digits in enumerate((1, 2, 17)):
            lines.append(b"f" * ((nl + k) % 16) + b"\n")                       # NO_COLON; slides what follows
            tail = (b"", b"|@0.5", b"|#tag:" + b"v" * (nl % 19), b"|@1|#t")[(nl + k) % 4]
            lines.append(b"n" * nl + b":" + b"7" * digits + b"|c" + tail + b"\n")
            lines.append(b"n" * nl + b":" + b"7" * digits + b"|x" + tail + b"\n")   # TYPE
    lines.append(b"last.line:1|c|#no.newline")
    data, recs, hashes = made_up(lines, 2)
    with Dev(pkg, torch, torch_stream, 2) as d:
        for mis in (0, 1, 7, 15):
            res, = d.run([(data, recs, hashes)], f"mis {mis}", mis=(mis, 0, 0))
            starts, colons, pipes, ends = set(), set(), set(), set()
            for x, ln in zip(recs, lines):
                a = mis + int(x["offset"])
                starts.add(a % 16)
                if b":" in ln:
                    colons.add((a + ln.index(b":")) % 16)
                    pipes.add((a + ln.index(b"|")) % 16)
                    ends.add((a + len(ln) - 1) % 16)
            assert starts == set(range(16)) and {15, 0, 1} <= colons and {15, 0, 1} <= pipes and {15, 0, 1} <= ends
            assert int(res.reason[-1]) == E.OK and int(recs[-1]["offset"]) + int(recs[-1]["length"]) == len(data)
            assert int(res.hits[E.OK, 0]) == 121 and int(res.hits[E.TYPE, 0]) == 120


def test_limits_of_numbers_sets_and_line_lengths(pkg, torch_stream):
    import torch

    d20, d21 = b"1" * 20, b"1" * 21
    lines = [b"a:" + d20 + b"|c\n", b"a:" + d21 + b"|c\n", b"a:1." + d20 + b"|g\n", b"a:1." + d21 + b"|g\n",
             b"a:" + d20 + b"." + d20 + b"|ms|@" + d20 + b"." + d20 + b"\n", b"a:1|c|@" + d21 + b"\n", b"a:1|c|@0." + d21 + b"\n",
             b"a:" + b"v" * 64 + b"|s\n", b"a:" + b"v" * 65 + b"|s\n", b"a:" + b"v" * 64 + b"|s|#t\n",
             b"n" * 1448 + b"\n", b"n" * 1449, b"n" * 1443 + b":1|c\n", b"a:1|c|#" + b"t" * 1441 + b"\n",
             b"a:1|c|#" + b"t" * 1000 + b"\x80" + b"t" * 440 + b"\n", b"a:1|c|#" + b"t" * 1440 + b"|\n",
             b"n" * 800 + b"|" + b"n" * 600 + b":1|c\n", b"a:" + b"1" * 1400 + b"|c\n", b"a:1|c|@" + b"1" * 1400 + b"\n"]
    with Dev(pkg, torch, torch_stream, 2) as d:
        for mis in (0, 3):
            res, = d.run([made_up(lines, 2)], f"limits mis {mis}", mis=(mis, 0, 0))
            assert res.reason.tolist() == [0, 6, 0, 6, 0, 8, 8, 0, 6, 0, 1, 1, 0, 0, 9, 7, 3, 6, 8]


COUNTS = [0, 1, 255, 256, 257, 513]


@pytest.mark.parametrize("count", COUNTS)
def test_record_counts_around_the_tile(pkg, torch_stream, count):
    import torch

    with Dev(pkg, torch, torch_stream, 3) as d:
        res, = d.run([mix(7 + count, count, 3)], str(count))
        assert int(res.counts[0] + res.counts[1]) == count
        if count >= 255:
            assert int(res.counts[1]) > 20 and len(set(res.reason.tolist())) >= 8


@pytest.mark.parametrize("mask,types", [(0, E.TYPES_ALL), (E.DROP_ALL, E.TYPES_ALL), (1 << E.VALUE, E.TYPES_ALL),
                                        (1 << E.NO_COLON, E.TYPES_ALL), (1 << E.TAGS, E.TYPES_ALL),
                                        ((1 << E.TYPE) | (1 << E.RATE), 1 | 2), (E.DROP_ALL, 4 | 16)])
def test_drop_masks_and_type_subsets(pkg, torch_stream, mask, types):
    import torch

    lines = [POOL[k % len(POOL)] + b"\n" for k in range(600)]
    with Dev(pkg, torch, torch_stream, 3, mask, types) as d:
        res, = d.run([made_up(lines, 3)], f"mask {mask:#x} types {types}")
        assert int(res.counts[3]) == 600
        if mask == 0:
            assert int(res.counts[1]) == 0
        if types != E.TYPES_ALL:
            assert int(res.hits[E.TYPE, 0]) > 100


def test_every_line_is_ok(pkg, torch_stream):
    """Hits equal the line count exactly (the wave settles the run before any atomic)."""
    import torch

    k = 3 * pkg.VALIDATE_TILE + 17
    with Dev(pkg, torch, torch_stream, 4) as d:
        res, = d.run([E.records_of([b"the.one.name:%d|c" % i for i in range(k)], 4)], "all ok")
        nbytes = sum(len(b"the.one.name:%d|c\n" % i) for i in range(k))
        assert res.hits.tolist() == [[k, nbytes]] + [[0, 0]] * 9 and res.counts.tolist() == [k, 0, 0, k]


def test_hostile_and_overlapping_records_pass_through(pkg, torch_stream):
    import torch

    data = b"debug.a:1|c\ndebug.b:22|c\n"
    rng = np.random.default_rng(8)
    recs = np.zeros(700, E.RECORD_DTYPE)
    recs["offset"] = rng.choice([0, 1, 12, 20, 24, 25, 26, 1 << 20, 0xFFFFFFFF, 0xFFFFFFF0], 700)
    recs["length"] = rng.choice([0, 1, 2, 7, 12, 13, 25, 26, 1449, 0xFFFF], 700)
    recs["route"] = rng.choice([0, 1, 2, 3, 0xFFFC, 0xFFFD, 0xFFFE, 0xFFFF, 77], 700)
    with Dev(pkg, torch, torch_stream, 2) as d:
        for mis in (0, 9):
            res, = d.run([(data, recs, rng.integers(0, 1 << 62, 700).astype(np.uint64))], "hostile", mis=(mis, 0, 0))
            ns = res.reason == E.NOT_SUBJECT
            assert 200 < int(ns.sum()) < 690 and int(res.counts[1]) > 5 and int(res.counts[0]) >= int(ns.sum())


def test_clamped_device_counts(pkg, torch_stream):
    import torch

    data, recs, hashes = mix(12, 600, 3)
    with Dev(pkg, torch, torch_stream, 3) as d:
        for n_records, max_records in ((1 << 40, 300), (257, 600), (0, 600), (600, 0)):
            spec = dict(data=data, recs=recs, hashes=hashes, n_records=n_records, max_records=max_records)
            res, = d.run([spec], f"n {n_records} max {max_records}")
            assert int(res.counts[0] + res.counts[1]) == min(n_records, max_records)


@pytest.mark.parametrize("hashes,reason", [(False, False), (True, False), (False, True)], ids=["none", "hashes", "reason"])
def test_optional_pointers_and_odd_alignments(pkg, torch_stream, hashes, reason):
    import torch

    with Dev(pkg, torch, torch_stream, 3) as d:
        for mis in ((0, 0, 0), (1, 4, 8), (7, 4, 8), (13, 0, 8)):
            d.run([mix(20, 515, 3)], f"mis {mis}", mis=mis, hashes=hashes, reason=reason)


def test_32_batches_with_empty_ones_three_calls_then_reset(pkg, torch_stream):
    import torch

    sizes = [0, 1, 255, 256, 257, 0, 513, 3] * 4
    with Dev(pkg, torch, torch_stream, 4) as d:
        batches = d.upload([mix(30 + j, s, 4) for j, s in enumerate(sizes)])
        arr = d.r.validate_batches([b.tuple() for b in batches])
        for _ in range(3):
            d.r.validate(arr)
        res = d.check(batches, "32 batches", calls=3)      # the hits of three calls
        assert sum(int(x.counts[1]) for x in res) > 100
        d.r.validate_reset()
        d.hits[:] = 0
        d.r.validate(arr)
        d.check(batches, "after the reset")


def test_graph_capture_and_replay(pkg, torch_stream):
    import torch

    with Dev(pkg, torch, torch_stream, 3) as d:
        batches = d.upload([mix(50, 700, 3), mix(51, 100, 3)])
        arr = d.r.validate_batches([b.tuple() for b in batches])
        d.r.validate(arr)                                   # sizes the scratch
        d.check(batches, "eager")
        for b in batches:
            for x in (b.out, b.hout, b.reason, b.counts):
                x.fill()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch_stream):
            d.r.validate(arr)
        g.replay()
        g.replay()
        d.check(batches, "replayed", calls=2)


def test_argument_errors(pkg, torch_stream):
    import torch

    r = pkg.Router(2, 1 << 16)
    r.set_stream(torch_stream.cuda_stream)
    b, = [DevBatch(torch, dict(zip(("data", "recs", "hashes"), mix(1, 10, 2))))]
    ok = list(b.tuple())

    def rc(t, count=1):
        return pkg.lib().sr_validate(r._h, r.validate_batches([tuple(t)]), count)

    assert rc(ok) == -errno.EINVAL                          # the stage is not open
    for mask, types in ((1, 63), (1 << 10, 63), (0, 0), (0, 64)):
        with pytest.raises(pkg.SrError) as ei:
            r.validate_open(pkg.ValidateConfig(mask, types))
        assert ei.value.errno == errno.EINVAL
    with pytest.raises(pkg.SrError):
        r.validate_read()
    r.validate_open(pkg.ValidateConfig(E.DROP_ALL))
    with pytest.raises(pkg.SrError) as ei:
        r.validate_open(pkg.ValidateConfig(0))
    assert ei.value.errno == errno.EBUSY
    assert rc(ok, 0) == -errno.EINVAL and rc(ok, 33) == -errno.EINVAL
    for at in (0, 2, 3, 5, 9):                              # d_bytes, d_recs, d_n_records, d_out, d_counts
        bad = list(ok)
        bad[at] = 0
        assert rc(bad) == -errno.EINVAL, at
    bad = list(ok); bad[5] = ok[2]                          # d_out == d_recs
    assert rc(bad) == -errno.EINVAL
    bad = list(ok); bad[7] = ok[6]                          # d_hashes_out == d_hashes
    assert rc(bad) == -errno.EINVAL
    bad = list(ok); bad[9] = ok[3]                          # d_counts == d_n_records
    assert rc(bad) == -errno.EINVAL
    bad = list(ok); bad[1] = 0xFFFFFFF1
    assert rc(bad) == -errno.EINVAL
    bad = list(ok); bad[4] = 0xFFFFFFF1
    assert rc(bad) == -errno.EINVAL
    torch.cuda.synchronize()
    b.out.expect(b"", "nothing was launched")
    assert r.validate_read().sum() == 0 and len(r.validate_read()) == E.REASONS and len(r.validate_read(2)) == 2
    r.validate_close()
    r.close()


@pytest.mark.parametrize("alive", [[1, 1, 1, 1, 1], [1, 1, 0, 1, 1]], ids=["all-alive", "one-dead"])
def test_route_validate_rules_coalesce_pack_payloads(pkg, torch_stream, alive):
    """The chain on one seeded batch of a few hundred lines: the route launch's records through sr_validate,
    sr_rules and sr_coalesce are the restatements composed in that order (records, hashes, counts, merged text);
    the packing and the payloads of the chain's result equal those of the restatement's records, uploaded."""
    import torch
    import coalesce_expect as CE
    import rules_expect as RE

    n = 5
    rng = np.random.default_rng(99)
    pool = POOL + [b"debug.x:1|c", b"debug.y:2|c", b"hot.counter:1|c", b"hot.counter:3|c", b"hot.other:2|c", b"debug.bad:x|c"]
    lines = [pool[k] for k in rng.integers(0, len(pool), 400)]
    data = b"".join(x + b"\n" for x in lines)
    rules = [(b"debug.", RE.PREFIX, RE.DROP)]
    nb, cap = len(data), len(data)
    mp = pkg.max_packets(2 * nb, n)
    z = lambda k, dt=torch.int64: torch.zeros(max(k, 1), dtype=dt, device="cuda")
    p = lambda t: t.data_ptr()
    with Dev(pkg, torch, torch_stream, n) as d:
        r = d.r
        r.set_alive(alive)
        r.rules_open(pkg.RuleSet(rules))
        r.coalesce_open(0)
        d_bytes = torch.zeros(2 * nb, dtype=torch.uint8, device="cuda")
        d_bytes[:nb].copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
        d_recs, d_hash, d_vout, d_vh, d_rout, d_rh, d_cout = (z(cap) for _ in range(7))
        d_n, d_vc, d_rc, d_cc = z(1), z(4), z(4), z(4)
        d_pd = z((n + 63) // 64)
        r.route_device_many([(p(d_bytes), nb, p(d_recs), cap, p(d_hash), p(d_n), p(d_pd))])
        r.validate([(p(d_bytes), nb, p(d_recs), p(d_n), cap, p(d_vout), p(d_hash), p(d_vh), 0, p(d_vc))])
        r.rules([(p(d_bytes), nb, p(d_vout), p(d_vc), cap, p(d_rout), p(d_vh), p(d_rh), 0, p(d_rc))])
        r.coalesce([(p(d_bytes), nb, nb, p(d_rout), p(d_rc), cap, p(d_rh), p(d_cout), p(d_cc))])
        torch.cuda.synchronize()
        nrec = int(d_n.cpu().numpy()[0])
        recs = d_recs.cpu().numpy().view(E.RECORD_DTYPE)[:nrec].copy()
        hashes = d_hash.cpu().numpy().view(np.uint64)[:nrec].copy()
        assert nrec == len(lines)
        v = E.apply(data, recs, hashes, n, E.DROP_ALL)
        u = RE.apply(data, v.out, v.hashes_out, n, rules)
        w = CE.coalesce(data, u.out, u.hashes_out, n, CE.DEFAULT_SLOTS, nb)
        assert d_vc.cpu().numpy().view(np.uint64).tolist() == v.counts.tolist() and int(v.counts[1]) > 50
        assert np.array_equal(d_vout.cpu().numpy().view(E.RECORD_DTYPE)[: len(v.out)], v.out)
        assert np.array_equal(d_vh.cpu().numpy().view(np.uint64)[: len(v.out)], v.hashes_out)
        assert d_rc.cpu().numpy().view(np.uint64).tolist() == u.counts.tolist() and int(u.counts[1]) > 10
        assert np.array_equal(d_rout.cpu().numpy().view(E.RECORD_DTYPE)[: len(u.out)], u.out)
        assert int(u.hits[0, 0]) < sum(x.startswith(b"debug.") for x in lines)   # debug.bad:x|c never reached the rules
        assert d_cc.cpu().numpy().view(np.uint64).tolist() == w.counts.tolist() and int(w.counts[2]) >= 1
        text = bytes(d_bytes[nb: nb + int(w.counts[3])].cpu().numpy())
        assert text == w.text
        got_recs = d_cout.cpu().numpy().view(E.RECORD_DTYPE)[: int(w.counts[0])].copy()
        assert np.array_equal(got_recs, w.out)

        def packed(src, cnt):
            d_srt, d_pk, d_counts = z(cap), z(2 * mp), z(4)
            d_fin, d_fout = z(n, torch.int16), z(n, torch.int16)
            r.pack_packets_many([(p(src), p(cnt), cap, p(d_fin), p(d_pd), p(d_srt), p(d_pk), mp, p(d_counts), p(d_fout))])
            pay_cap = 2 * nb + 1450 * n
            d_pay, d_off, d_tot = z(pay_cap, torch.uint8), z(mp + 1, torch.int32), z(1)
            r.pack_payloads((p(d_bytes), 2 * nb, p(d_srt), cap, p(d_pk), mp, p(d_counts), p(d_fout), 0, 0, p(d_pay), pay_cap,
                             p(d_off), p(d_tot)))
            torch.cuda.synchronize()
            c = d_counts.cpu().numpy()
            total = int(d_tot.cpu().numpy()[0])
            assert 0 < total <= pay_cap
            return (c.tolist(), d_srt.cpu().numpy()[: int(c[2])].tolist(), d_pk.cpu().numpy()[: 2 * int(c[0])].tolist(),
                    d_fout.cpu().numpy().tolist(), d_off.cpu().numpy()[: int(c[0]) + 1].tolist(), total,
                    d_pk.cpu().numpy().view(np.uint16).reshape(-1, 8)[: int(c[0])].copy(), d_pay.cpu().numpy()[:total].tobytes())

        got = packed(d_cout, d_cc)
        e_recs = torch.from_numpy(np.ascontiguousarray(w.out).view(np.int64).copy()).cuda() if len(w.out) else z(1)
        e_src = z(cap)
        e_src[: len(w.out)].copy_(e_recs[: len(w.out)])
        e_cnt = torch.from_numpy(np.array([len(w.out)], np.int64)).cuda()
        want = packed(e_src, e_cnt)
        assert got[:6] == want[:6] and got[0][0] > 0
        for q, pk in enumerate(got[6]):   # (room left for a carry is not written: the bytes of this batch's lines)
            lo = got[4][q] + int(pk[5])
            assert got[7][lo: lo + int(pk[4])] == want[7][lo: lo + int(pk[4])], q
