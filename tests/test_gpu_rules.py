"""GPU: sr_rules, the name rules on the device, against tests/rules_expect.py. Records and hashes come from the
restatement's own tokeniser or are made up, so the stage is driven alone. Every buffer lies between guard bytes
and is compared whole: the records out, the hashes out, the match indices and the room behind them, the four
counts, and the inputs, which must come back unchanged. The hits are compared exactly."""
from __future__ import annotations

import errno

import numpy as np
import pytest

import rules_expect as E
from rules_expect import DROP, EXACT, KEEP, PREFIX
from test_gpu_coalesce import Buf

pytestmark = pytest.mark.gpu

RULES = [(b"debug.", PREFIX, DROP), (b"debug.keep.", PREFIX, KEEP), (b"app.req", EXACT, DROP), (b"app.req", PREFIX, KEEP),
         (b"n\x00\xff", PREFIX, DROP), (b"x" * 64, EXACT, DROP)]


class DevBatch:
    def __init__(self, torch, spec, mis=(0, 0, 0), hashes=True, match=True):
        self.data, self.recs = bytes(spec["data"]), np.ascontiguousarray(spec["recs"], E.RECORD_DTYPE)
        self.hashes = np.ascontiguousarray(spec["hashes"], np.uint64)
        self.n_records = len(self.recs) if spec.get("n_records") is None else spec["n_records"]
        self.max_records = len(self.recs) if spec.get("max_records") is None else spec["max_records"]
        self.with_hashes, self.with_match = hashes, match
        mb, mr, m8 = mis
        self.bytes = Buf(torch, self.data, None, mb)
        self.d_recs = Buf(torch, self.recs.tobytes(), None, mr)
        self.d_hashes = Buf(torch, self.hashes.tobytes() if len(self.hashes) else bytes(8), None, m8)
        self.d_n = Buf(torch, np.asarray([self.n_records], np.uint64).tobytes(), None, m8)
        self.out = Buf(torch, b"", 8 * self.max_records, mr)
        self.hout = Buf(torch, b"", 8 * self.max_records, m8)
        self.match = Buf(torch, b"", 2 * self.max_records, 2 * (mr & 1))
        self.counts = Buf(torch, b"", 32, m8)

    def tuple(self):
        mr = self.max_records
        return (self.bytes.ptr if self.bytes.size else 0, len(self.data), self.d_recs.ptr if mr else 0, self.d_n.ptr, mr,
                self.out.ptr if mr else 0, self.d_hashes.ptr if self.with_hashes else 0,
                self.hout.ptr if self.with_hashes else 0, self.match.ptr if self.with_match else 0, self.counts.ptr)

    def check(self, n, rules, default, label):
        res = E.apply(self.data, self.recs, self.hashes, n, rules, default, self.n_records, self.max_records)
        self.counts.expect(res.counts.tobytes(), f"{label}: counts")
        self.out.expect(res.out.tobytes(), f"{label}: records out")
        self.hout.expect(res.hashes_out.tobytes() if self.with_hashes else b"", f"{label}: hashes out")
        self.match.expect(res.match.tobytes() if self.with_match else b"", f"{label}: match indices")
        self.bytes.expect(self.data, f"{label}: batch")
        self.d_recs.expect(self.recs.tobytes(), f"{label}: input records")
        self.d_hashes.expect(self.hashes.tobytes() if len(self.hashes) else bytes(8), f"{label}: hashes")
        self.d_n.expect(np.asarray([self.n_records], np.uint64).tobytes(), f"{label}: record count")
        return res


class Dev:
    """A context with the stage open on the test's stream."""

    def __init__(self, pkg, torch, stream, n, rules=RULES, default=KEEP, max_batch=1 << 20):
        self.pkg, self.torch, self.n, self.rule_list, self.default = pkg, torch, n, list(rules), default
        self.r = pkg.Router(n, max_batch)
        self.r.set_stream(stream.cuda_stream)
        self.r.rules_open(pkg.RuleSet(rules, default))
        self.hits = np.zeros((len(self.rule_list) + 1, 2), np.uint64)

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
        res = [b.check(self.n, self.rule_list, self.default, f"{label}[{j}]") for j, b in enumerate(batches)]
        for x in res:
            self.hits += x.hits * np.uint64(calls)
        got = self.r.rules_read()
        assert got.tolist() == self.hits.tolist(), f"{label}: hits"
        return res

    def run(self, specs, label, **kw):
        batches = self.upload(specs, **kw)
        self.r.rules([b.tuple() for b in batches])
        return self.check(batches, label)


def mix(seed, count, n):
    """`count` lines: names that the rules drop and keep, other names, and the kinds of unrouted lines."""
    rng = np.random.default_rng(seed)
    names = [b"debug.a", b"debug.keep.b", b"debug.kee", b"app.req", b"app.req.count", b"app.re", b"sys.cpu", b"n\x00\xffz",
             b"n\x00", b"x" * 64, b"x" * 63]
    lines = []
    for u, k, v in zip(rng.random(count), rng.integers(0, len(names), count), rng.integers(0, 3000, count)):
        if u < 0.88:
            lines.append(names[k] + b":%d|c" % v)
        elif u < 0.92:
            lines.append(b"ab")                       # invalid length
        elif u < 0.96:
            lines.append(b"debug.no colon here")      # invalid format: begins like a rule, not subject
        else:
            lines.append(names[k] + b".t:%d|ms|@0.1" % v)
    return E.records_of(lines, n)


COUNTS = [0, 1, 255, 256, 257, 513]


@pytest.mark.parametrize("count", COUNTS)
def test_record_counts_around_the_tile(pkg, torch_stream, count):
    import torch

    with Dev(pkg, torch, torch_stream, 3) as d:
        res, = d.run([mix(7 + count, count, 3)], str(count))
        assert int(res.counts[0] + res.counts[1]) == count
        if count >= 255:
            assert int(res.counts[1]) > 20 and len(set(res.match.tolist())) >= 6


@pytest.mark.parametrize("plen", [1, 15, 16, 17, 63, 64])
def test_pattern_lengths_and_every_head_offset(pkg, torch_stream, plen):
    """A pattern of plen bytes as PREFIX and EXACT; names of plen - 1, plen and plen + 1 bytes and one that differs
    in its last byte, each at every offset mod 16 (fillers of 0..15 bytes slide the heads), in a batch whose own
    address is moved by 0..3 bytes. The last line of the batch matches: its head ends with the batch."""
    import torch

    pat = bytes(65 + (i % 26) for i in range(plen))
    rules = [(pat, PREFIX, DROP), (pat, EXACT, KEEP), (pat[:1] + b"\x00", PREFIX, DROP)]
    names = [pat, pat + b"z", pat[:-1] + b"!", pat[:1] + b"\x00q"] + ([pat[:-1]] if plen > 1 else [])
    lines = []
    for k in range(48):
        lines.append(b"f" * 5 + b":" + b"1" * (k % 16))     # not matched; moves the next heads through every residue
        for nm in names:
            lines.append(nm + b":1|c")
    lines.append(pat + b"tail:1|g")
    for mis in (0, 1, 3):
        with Dev(pkg, torch, torch_stream, 2, rules) as d:
            data, recs, hashes = E.records_of(lines, 2)
            res, = d.run([(data, recs, hashes)], f"plen {plen} mis {mis}", mis=(mis, 0, 0))
            assert {int(o) % 16 for o in recs["offset"]} == set(range(16))
            assert int(res.match[-1]) == 0 and int(recs[-1]["offset"]) + int(recs[-1]["length"]) == len(data)
            assert int(res.hits[0, 0]) >= 49 and int(res.hits[1, 0]) == 48 and int(res.hits[2, 0]) == 48


def test_a_matching_head_that_ends_the_batch_and_short_lines(pkg, torch_stream):
    """Lines shorter than their pattern, a PREFIX with p = L - 1 as the batch's last bytes, an EXACT whose ':' is
    the byte before the last, and records made up over one small batch: nothing behind nbytes is read (the guard
    bytes behind the batch would complete a longer pattern)."""
    import torch

    rules = [(b"abcdefgh", PREFIX, DROP), (b"abcdefghij", PREFIX, KEEP), (b"abc", EXACT, DROP)]
    data = b"abc:\nabcdefg\nab\nabcdefgh\n"
    recs = np.array([(0, 5, 0), (5, 8, 0), (13, 3, 0), (16, 9, 0), (16, 8, 1), (0, 4, 0), (0, 2, 1), (24, 1, 0),
                     (17, 8, 0), (16, 10, 0), (25, 0, 0), (0, 5, 7)], E.RECORD_DTYPE)
    with Dev(pkg, torch, torch_stream, 2, rules) as d:
        res, = d.run([(data, recs, np.arange(len(recs), dtype=np.uint64))], "edges")
        assert res.match.tolist() == [2, 3, 3, 0, 3, 3, 3, 3, 3, 0xFFFF, 0xFFFF, 0xFFFF]


def test_nested_prefixes_and_the_tie_across_a_tile_boundary(pkg, torch_stream):
    import torch

    R = pkg.RULES_TILE
    rules = [(b"a.", PREFIX, DROP), (b"a.b.", PREFIX, KEEP), (b"a.b.c", EXACT, DROP), (b"a.b.c", PREFIX, DROP),
             (b"a.b.c.d.", PREFIX, KEEP)]
    lines = [b"filler.%d:1|c" % i for i in range(2 * R + 9)]
    cases = [b"a.x:1|c", b"a.b.x:1|c", b"a.b.c:1|c", b"a.b.cc:1|c", b"a.b.c.d.e:1|c", b"a.b.c.d:1|c", b"a:1|c"]
    for k, c in enumerate(cases):
        lines[R - 3 + k] = c
        lines[2 * R - 4 + k] = c
    with Dev(pkg, torch, torch_stream, 4, rules) as d:
        res, = d.run([E.records_of(lines, 4)], "nested")
        assert res.match[R - 3: R + 4].tolist() == [0, 1, 2, 3, 4, 3, 5] == res.match[2 * R - 4: 2 * R + 3].tolist()


def test_all_256_rules_and_4096_text_bytes(pkg, torch_stream):
    import torch

    rules = [(b"%02x" % i + bytes([33 + (i * 7 + q) % 90 for q in range(14)]), (PREFIX, EXACT)[i & 1], (DROP, KEEP)[(i >> 1) & 1])
             for i in range(256)]
    rules = [(p.replace(b":", b";"), k, a) for p, k, a in rules]
    assert sum(len(p) for p, _, _ in rules) == 4096 and E.check(rules)
    lines = []
    for i in range(256):
        lines += [rules[i][0] + b":1|c", rules[i][0] + b"x:1|c", rules[i][0][:-1] + b":1|c"]
    with Dev(pkg, torch, torch_stream, 5, rules) as d:
        res, = d.run([E.records_of(lines, 5)], "256 rules")
        assert (res.hits[:256, 0] >= 1).all() and int(res.hits[256, 0]) >= 256
        big = [(bytes([65 + i % 26]) + b"%02d" % i + b"y" * 61, PREFIX, DROP) for i in range(64)]
    with Dev(pkg, torch, torch_stream, 5, big) as d:   # 64 patterns of 64 bytes: 4096 too
        res, = d.run([E.records_of([big[i % 64][0] + b":%d|c" % i for i in range(300)], 5)], "64 x 64")
        assert res.counts.tolist()[:2] == [0, 300]


@pytest.mark.parametrize("default", [KEEP, DROP])
def test_no_rules(pkg, torch_stream, default):
    import torch

    with Dev(pkg, torch, torch_stream, 3, [], default) as d:
        res, = d.run([mix(3, 600, 3)], "no rules")
        assert int(res.counts[1]) == (0 if default == KEEP else int(res.counts[3])) and int(res.counts[3]) > 400


def test_default_drop_is_an_allow_list(pkg, torch_stream):
    import torch

    with Dev(pkg, torch, torch_stream, 3, [(b"app.", PREFIX, KEEP), (b"sys.cpu", EXACT, KEEP)], DROP) as d:
        res, = d.run([mix(4, 700, 3)], "allow list")
        assert 0 < int(res.hits[0, 0]) and 0 < int(res.hits[1, 0]) and int(res.counts[1]) == int(res.hits[2, 0]) > 100


@pytest.mark.parametrize("action", [DROP, KEEP])
def test_every_line_hits_one_rule(pkg, torch_stream, action):
    """Hits equal the line count exactly (the wave settles the run before any atomic), every line kept or every
    line dropped."""
    import torch

    k = 3 * pkg.RULES_TILE + 17
    rules = [(b"the.one.name", EXACT, action), (b"never", PREFIX, DROP)]
    with Dev(pkg, torch, torch_stream, 4, rules) as d:
        res, = d.run([E.records_of([b"the.one.name:%d|c" % i for i in range(k)], 4)], "one rule")
        nbytes = sum(len(b"the.one.name:%d|c\n" % i) for i in range(k))
        assert res.hits.tolist() == [[k, nbytes], [0, 0], [0, 0]]
        assert res.counts.tolist() == ([0, k, nbytes, k] if action == DROP else [k, 0, 0, k])


def test_hostile_and_overlapping_records_pass_through(pkg, torch_stream):
    import torch

    data = b"debug.a:1|c\ndebug.b:22|c\n"
    rng = np.random.default_rng(8)
    recs = np.zeros(700, E.RECORD_DTYPE)
    recs["offset"] = rng.choice([0, 1, 12, 20, 24, 25, 26, 1 << 20, 0xFFFFFFFF, 0xFFFFFFF0], 700)
    recs["length"] = rng.choice([0, 1, 2, 7, 12, 13, 25, 26, 1449, 0xFFFF], 700)
    recs["route"] = rng.choice([0, 1, 2, 3, 0xFFFC, 0xFFFD, 0xFFFE, 0xFFFF, 77], 700)
    with Dev(pkg, torch, torch_stream, 2, [(b"debug.", PREFIX, DROP), (b"ebug.a", EXACT, DROP)]) as d:
        res, = d.run([(data, recs, rng.integers(0, 1 << 62, 700).astype(np.uint64))], "hostile")
        ns = res.match == E.NOT_SUBJECT
        assert 200 < int(ns.sum()) < 690 and int(res.counts[1]) > 5 and int(res.counts[0]) >= int(ns.sum())


def test_clamped_device_counts(pkg, torch_stream):
    import torch

    data, recs, hashes = mix(12, 600, 3)
    with Dev(pkg, torch, torch_stream, 3) as d:
        for n_records, max_records in ((1 << 40, 300), (257, 600), (0, 600), (600, 0)):
            spec = dict(data=data, recs=recs, hashes=hashes, n_records=n_records, max_records=max_records)
            res, = d.run([spec], f"n {n_records} max {max_records}")
            assert int(res.counts[0] + res.counts[1]) == min(n_records, max_records)


@pytest.mark.parametrize("hashes,match", [(False, False), (True, False), (False, True)], ids=["none", "hashes", "match"])
def test_optional_pointers_and_odd_alignments(pkg, torch_stream, hashes, match):
    import torch

    with Dev(pkg, torch, torch_stream, 3) as d:
        for mis in ((0, 0, 0), (1, 4, 8), (7, 4, 8), (13, 0, 8)):
            d.run([mix(20, 515, 3)], f"mis {mis}", mis=mis, hashes=hashes, match=match)


def test_32_batches_with_empty_ones_three_calls_then_reset(pkg, torch_stream):
    import torch

    sizes = [0, 1, 255, 256, 257, 0, 513, 3] * 4
    with Dev(pkg, torch, torch_stream, 4) as d:
        batches = d.upload([mix(30 + j, s, 4) for j, s in enumerate(sizes)])
        arr = d.r.rules_batches([b.tuple() for b in batches])
        for _ in range(3):
            d.r.rules(arr)
        res = d.check(batches, "32 batches", calls=3)      # the hits of three calls
        assert sum(int(x.counts[1]) for x in res) > 100
        d.r.rules_reset()
        d.hits[:] = 0
        d.r.rules(arr)
        d.check(batches, "after the reset")


def test_graph_capture_and_replay(pkg, torch_stream):
    import torch

    with Dev(pkg, torch, torch_stream, 3) as d:
        batches = d.upload([mix(50, 700, 3), mix(51, 100, 3)])
        arr = d.r.rules_batches([b.tuple() for b in batches])
        d.r.rules(arr)                                      # sizes the scratch
        d.check(batches, "eager")
        for b in batches:
            for x in (b.out, b.hout, b.match, b.counts):
                x.fill()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch_stream):
            d.r.rules(arr)
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
        return pkg.lib().sr_rules(r._h, r.rules_batches([tuple(t)]), count)

    assert rc(ok) == -errno.EINVAL                          # the stage is not open
    with pytest.raises(pkg.SrError):
        r.rules_open(pkg.RuleSet([(b"a:b", PREFIX, DROP)]))
    with pytest.raises(pkg.SrError):
        r.rules_read()
    r.rules_open(pkg.RuleSet(RULES))
    with pytest.raises(pkg.SrError) as ei:
        r.rules_open(pkg.RuleSet(RULES))
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
    assert r.rules_read().sum() == 0 and len(r.rules_read()) == len(RULES) + 1 and len(r.rules_read(2)) == 2
    r.rules_close()
    r.close()


def test_route_rules_pack_equals_the_pipeline_fed_the_kept_lines(pkg, oracle, torch_stream):
    """Route -> rules -> pack against route -> pack of a batch that holds the kept lines only: the same lines in
    the same packets (every field), the same payload bytes, offsets and total from sr_pack_payloads; the records'
    offsets differ, so the records are compared through their bytes."""
    import torch

    n = 5
    data, recs, hashes = mix(77, 2000, n)
    res = E.apply(data, recs, hashes, n, RULES)   # lines that are not routed are not subject: they stay
    kept = b"".join(data[int(x["offset"]): int(x["offset"]) + int(x["length"])] for x in res.out)
    assert 0 < len(kept) < len(data)

    def packed(r, batch, rules_on):
        nb, cap = len(batch), len(batch)
        mp = pkg.max_packets(nb, n)
        z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device="cuda")
        d_bytes = torch.from_numpy(np.frombuffer(batch, np.uint8).copy()).cuda()
        d_recs, d_hash, d_rout, d_srt = (z(cap, torch.int64) for _ in range(4))
        d_n, d_rc, d_counts = z(1, torch.int64), z(4, torch.int64), z(4, torch.int64)
        d_pd, d_pk = z((n + 63) // 64, torch.int64), z(2 * mp, torch.int64)
        d_fin, d_fout = z(n, torch.int16), z(n, torch.int16)
        p = lambda t: t.data_ptr()
        r.route_device_many([(p(d_bytes), nb, p(d_recs), cap, p(d_hash), p(d_n), p(d_pd))])
        src, cnt = d_recs, d_n
        if rules_on:
            r.rules([(p(d_bytes), nb, p(d_recs), p(d_n), cap, p(d_rout), 0, 0, 0, p(d_rc))])
            src, cnt = d_rout, d_rc
        r.pack_packets_many([(p(src), p(cnt), cap, p(d_fin), p(d_pd), p(d_srt), p(d_pk), mp, p(d_counts), p(d_fout))])
        pay_cap = nb + 1450 * n
        d_pay, d_off, d_tot = z(pay_cap, torch.uint8), z(mp + 1, torch.int32), z(1, torch.int64)
        r.pack_payloads((p(d_bytes), nb, p(d_srt), cap, p(d_pk), mp, p(d_counts), p(d_fout), 0, 0, p(d_pay), pay_cap,
                         p(d_off), p(d_tot)))
        torch.cuda.synchronize()
        c = d_counts.cpu().numpy()
        srt = d_srt.cpu().numpy().view(E.RECORD_DTYPE)[: int(c[2])]
        pk = d_pk.cpu().numpy().view(np.uint8).reshape(-1, 16)[: int(c[0])]
        text = [batch[int(x["offset"]): int(x["offset"]) + int(x["length"])] for x in srt]
        total = int(d_tot.cpu().numpy()[0])
        assert 0 < total <= pay_cap
        payload = (d_pay.cpu().numpy()[:total].tobytes(), d_off.cpu().numpy()[: int(c[0]) + 1].tolist(), total)
        return text, srt["route"].tolist(), pk, d_fout.cpu().numpy().tolist(), c.tolist(), payload

    with Dev(pkg, torch, torch_stream, n) as d:
        d.r.set_alive([1] * n)
        got = packed(d.r, data, True)
        want = packed(d.r, kept, False)
    assert got[0] == want[0] and got[1] == want[1] and got[3] == want[3] and got[4] == want[4]
    # a packet is {first sorted record, lines, shard, length, carry, open}: no byte offset in it, so every field is
    # equal; and the payload stage gathers the same bytes to the same places
    assert np.array_equal(got[2], want[2]) and len(got[2]) > n
    assert got[5][1] == want[5][1] and got[5][2] == want[5][2]
    # (room left for a carry is not written: compare the bytes of this batch's lines, packet by packet)
    offs = got[5][1]
    pk = got[2].view(np.uint16).reshape(-1, 8)   # first lo, first hi, nlines, shard, length, carry, open lo, open hi
    for q in range(len(pk)):
        lo = offs[q] + int(pk[q][5])
        assert got[5][0][lo: lo + int(pk[q][4])] == want[5][0][lo: lo + int(pk[q][4])], q


def test_route_rules_coalesce_a_dropped_counter_is_never_merged(pkg, torch_stream):
    import torch
    import coalesce_expect as CE

    n = 3
    lines = [b"debug.hot:1|c", b"app.hot:2|c"] * 300 + [b"sys.cpu:3|c"] * 5
    data, recs, hashes = E.records_of(lines, n)
    rules = [(b"debug.", PREFIX, DROP)]
    with Dev(pkg, torch, torch_stream, n, rules) as d:
        d.r.coalesce_open(0)
        nb, cap = len(data), len(recs)
        d_bytes = torch.zeros(2 * nb, dtype=torch.uint8, device="cuda")
        d_bytes[:nb].copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
        d_recs, d_hash, d_n = up(recs), up(hashes), up(np.array([cap], np.uint64))
        z = lambda k: torch.zeros(k, dtype=torch.int64, device="cuda")
        d_rout, d_rh, d_rc, d_cout, d_cc = z(cap), z(cap), z(4), z(cap), z(4)
        p = lambda t: t.data_ptr()
        d.r.rules([(p(d_bytes), nb, p(d_recs), p(d_n), cap, p(d_rout), p(d_hash), p(d_rh), 0, p(d_rc))])
        d.r.coalesce([(p(d_bytes), nb, nb, p(d_rout), p(d_rc), cap, p(d_rh), p(d_cout), p(d_cc))])
        torch.cuda.synchronize()
        res = E.apply(data, recs, hashes, n, rules)
        assert d_rc.cpu().numpy().tolist() == res.counts.tolist() and int(res.counts[1]) == 300
        assert np.array_equal(d_rh.cpu().numpy().view(np.uint64)[:305], res.hashes_out)
        want = CE.coalesce(data, res.out, res.hashes_out, n, CE.DEFAULT_SLOTS, nb)
        assert d_cc.cpu().numpy().tolist() == want.counts.tolist() and int(want.counts[2]) == 2
        text = bytes(d_bytes[nb: nb + int(want.counts[3])].cpu().numpy())
        assert text == want.text and b"debug" not in text and b"app.hot:600|c\n" in text
