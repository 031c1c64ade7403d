"""GPU: sr_sample, the sample rates on the device, against tests/sample_expect.py. Records and hashes come from the
restatement's own tokeniser or are made up, so the stage is driven alone. Every buffer lies between guard bytes and
is compared whole: the batch with the rewritten text and the room behind it, the records out, the hashes out, the
steps, the four counts, and the inputs, which must come back unchanged. The hits are compared exactly."""
from __future__ import annotations

import errno

import numpy as np
import pytest

import sample_expect as E
from stats_expect import fmix64_inverse
from test_gpu_coalesce import Buf

pytestmark = pytest.mark.gpu


def made_up(lines, n, hashes=None):
    """The lines laid end to end exactly as given (a '\\n' only where the line has one), a record per line and,
    unless given, the hash of what stands before the first ':'."""
    data = b"".join(lines)
    recs = np.zeros(len(lines), E.RECORD_DTYPE)
    lens = np.array([len(x) for x in lines], np.int64)
    recs["offset"] = np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(lines) else []
    recs["length"] = lens
    recs["route"] = np.arange(len(lines)) % n
    if hashes is None:
        hashes = [E.name_hash(x.split(b":")[0]) for x in lines]
    return data, recs, np.asarray(hashes, np.uint64)


class DevBatch:
    def __init__(self, torch, spec, mis=(0, 0, 0), hashes_out=True, step=True):
        self.data, self.recs = bytes(spec["data"]), np.ascontiguousarray(spec["recs"], E.RECORD_DTYPE)
        self.hashes = np.ascontiguousarray(spec["hashes"], np.uint64)
        self.n_records = len(self.recs) if spec.get("n_records") is None else spec["n_records"]
        self.max_records = len(self.recs) if spec.get("max_records") is None else spec["max_records"]
        self.cap = E.append_capacity(len(self.data)) if spec.get("append_cap") is None else spec["append_cap"]
        self.seed_add = spec.get("seed_add", 0)
        self.with_hashes, self.with_step = hashes_out, step
        mb, mr, m8 = mis
        self.bytes = Buf(torch, self.data, len(self.data) + self.cap, mb)   # the batch, then the room for the text
        self.d_recs = Buf(torch, self.recs.tobytes(), None, mr)
        self.d_hashes = Buf(torch, self.hashes.tobytes() if len(self.hashes) else bytes(8), None, m8)
        self.d_n = Buf(torch, np.asarray([self.n_records], np.uint64).tobytes(), None, m8)
        self.out = Buf(torch, b"", 8 * self.max_records, mr)
        self.hout = Buf(torch, b"", 8 * self.max_records, m8)
        self.step = Buf(torch, b"", self.max_records, mb & 3)
        self.counts = Buf(torch, b"", 32, m8)

    def outputs(self):
        return self.bytes, self.out, self.hout, self.step, self.counts

    def tuple(self):
        mr = self.max_records
        return (self.bytes.ptr if self.bytes.size else 0, len(self.data), self.cap, self.d_recs.ptr if mr else 0, self.d_n.ptr,
                mr, self.d_hashes.ptr, self.out.ptr if mr else 0, self.hout.ptr if self.with_hashes else 0,
                self.step.ptr if self.with_step else 0, self.counts.ptr, self.seed_add)

    def check(self, d, label):
        res = E.apply(self.data, self.recs, self.hashes, d.n, d.limit, d.types, d.slots, (d.seed + self.seed_add) & E.M64,
                      self.n_records, self.max_records)
        self.counts.expect(res.counts.tobytes(), f"{label}: counts")
        self.step.expect(res.steps.tobytes() if self.with_step else b"", f"{label}: steps")
        self.out.expect(res.out.tobytes(), f"{label}: records out")
        self.hout.expect(res.hashes_out.tobytes() if self.with_hashes else b"", f"{label}: hashes out")
        self.bytes.expect(self.data + res.written(self.cap), f"{label}: batch and text")
        self.d_recs.expect(self.recs.tobytes(), f"{label}: input records")
        self.d_hashes.expect(self.hashes.tobytes() if len(self.hashes) else bytes(8), f"{label}: hashes")
        self.d_n.expect(np.asarray([self.n_records], np.uint64).tobytes(), f"{label}: record count")
        return res


class Dev:
    """A context with the stage open on the test's stream."""

    def __init__(self, pkg, torch, stream, n, limit, types=E.TYPES_ALL, slots=0, seed=0, max_batch=1 << 20):
        self.pkg, self.torch, self.n = pkg, torch, n
        self.limit, self.types, self.slots, self.seed = limit, types, slots, seed
        self.r = pkg.Router(n, max_batch)
        self.r.set_stream(stream.cuda_stream)
        self.r.sample_open(pkg.SampleConfig(limit, types, slots, seed))
        self.hits = np.zeros((E.STEPS, 2), np.uint64)

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
        res = [b.check(self, f"{label}[{j}]") for j, b in enumerate(batches)]
        for x in res:
            self.hits += x.hits * np.uint64(calls)
        got = self.r.sample_read()
        assert got.tolist() == self.hits.tolist(), f"{label}: hits"
        return res

    def run(self, specs, label, **kw):
        batches = self.upload(specs, **kw)
        self.r.sample([b.tuple() for b in batches])
        return self.check(batches, label)


POOL = [b"svc.t:12.5|ms", b"svc.t:7|ms|#env:prod,z:a", b"hot.h:1|h", b"hot.d:3.5|d|#t", b"cnt.c:1|c", b"cnt.c:2|c|#k:v",
        b"svc.t:1|ms|@0.5", b"g.x:+17|g", b"u:alice|s", b"no colon here", b":1|c", b"a:|ms", b"a:1", b"a:1|q", b"a:1|msx",
        b"a:1|", b"a:1|ms|", b"a:1|ms|x", b"ab", b"other.%d:1|ms"]


def mix(seed, count, n):
    """`count` lines, a few hot names among them, tokenised as the route launch would."""
    rng = np.random.default_rng(seed)
    return E.records_of([POOL[k] if k < len(POOL) - 1 else POOL[k] % rng.integers(0, 50)
                         for k in rng.integers(0, len(POOL), count)], n)


COUNTS = [0, 1, 255, 256, 257, 513]


@pytest.mark.parametrize("count", COUNTS)
def test_record_counts_around_the_tile(pkg, torch_stream, count):
    import torch

    with Dev(pkg, torch, torch_stream, 3, 2) as d:
        res, = d.run([mix(7 + count, count, 3)], str(count))
        assert int(res.counts[0] + res.counts[1]) == count
        if count >= 255:
            assert int(res.counts[1]) > 10 and int(res.counts[2]) >= 2 and (res.steps == E.NOT_SAMPLEABLE).sum() > 50


@pytest.mark.parametrize("slots", [0, 16])
def test_a_slots_members_in_different_workgroups(pkg, torch_stream, slots):
    """One hot name every third line of 1500: its members lie in six tiles and every wave holds other names too."""
    import torch

    lines = [b"the.hot.timer:%d|ms" % i if i % 3 == 0 else b"cold.%d:1|ms" % i for i in range(1500)]
    with Dev(pkg, torch, torch_stream, 4, 50, slots=slots) as d:
        res, = d.run([E.records_of(lines, 4)], "spread")
        hot = res.steps[::3] & 0x7F
        assert (hot == hot[0]).all() and hot[0] >= E.step(50, 500) >= 3 and int(res.counts[1]) > 300


def test_one_name_at_the_limit_and_one_over(pkg, torch_stream):
    import torch

    at = [b"at.limit:%d|ms" % i for i in range(40)]
    over = [b"over.limit:%d|ms" % i for i in range(41)]
    with Dev(pkg, torch, torch_stream, 2, 40) as d:
        res, = d.run([E.records_of(at + over, 2)], "limit")
        assert (res.steps[:40] == 0).all() and ((res.steps[40:] & 0x7F) == 1).all()
        assert res.hits[0].tolist() == [40, 40] and int(res.hits[1, 0]) == 41 and 5 < int(res.hits[1, 1]) < 36
        assert res.text.count(b"|@0.5\n") == int(res.counts[2]) == int(res.hits[1, 1])


def test_every_ladder_boundary_with_limit_1(pkg, torch_stream):
    """Names with exactly K[j] and K[j] + 1 lines for every step, and one with 12,000: every step is taken, the last
    one also beyond its bound. Each name has a slot of its own, so its count is its line count."""
    import torch

    sizes = sorted({k + e for k in E.K for e in (0, 1)} | {12000})
    lines, want = [], []
    for q, c in enumerate(sizes):
        lines += [b"name.%d:%d|h" % (q, i) for i in range(c)]
        want += [E.step(1, c)] * c
    order = np.random.default_rng(3).permutation(len(lines))
    lines, want = [lines[k] for k in order], np.array(want)[order]
    data, recs, hashes = E.records_of(lines, 3)
    assert len({E.fmix64(int(h)) & 0xFFFF for h in set(hashes.tolist())}) == len(sizes)
    with Dev(pkg, torch, torch_stream, 3, 1) as d:
        res, = d.run([(data, recs, hashes)], "ladder")
        assert np.array_equal(res.steps & 0x7F, want) and set(want.tolist()) == set(range(13))
        assert (res.hits[:, 0] > 0).all() and res.hits[0].tolist() == [1, 1]


def test_all_names_distinct(pkg, torch_stream):
    import torch

    with Dev(pkg, torch, torch_stream, 4, 2) as d:
        res, = d.run([E.records_of([b"distinct.%d:1|ms" % i for i in range(900)], 4)], "distinct")
        assert int(res.counts[0]) >= 890 and int(res.hits[0, 0]) >= 880


@pytest.mark.parametrize("names", [2, 3])
def test_names_that_share_a_slot_share_a_count(pkg, torch_stream, names):
    """S = 16 and made-up hashes that fall into slot 5: ten lines each, so the slot counts 10 * names."""
    import torch

    hs = [fmix64_inverse((0x1234567 * (k + 1)) << 4 | 5) for k in range(names)]
    lines = [b"n%d:%d|ms\n" % (i % names, i) for i in range(10 * names)] + [b"alone:1|ms\n"]
    hashes = [hs[i % names] for i in range(10 * names)] + [fmix64_inverse(0x70)]
    with Dev(pkg, torch, torch_stream, 2, 10, slots=16) as d:
        res, = d.run([made_up(lines, 2, hashes)], "shared")
        assert ((res.steps[:-1] & 0x7F) == names - 1).all() and E.step(10, 10 * names) == names - 1
        assert int(res.steps[-1]) == 0 and int(res.hits[names - 1, 0]) == 10 * names


KINDS = [b"t.c:1|c\n", b"t.ms:1|ms\n", b"t.h:1|h\n", b"t.d:1|d\n", b"t.tag:1|ms|#a:b,c\n", b"t.at:1|ms|@0.5\n",
         b"t.g:1|g\n", b"t\x00\xff\x80:\x00\xfe|ms|#\x00\xff\n", b"t.long:" + b"1" * 1431 + b"|h\n",
         b"t.longer:" + b"1" * 1430 + b"|h\n", b"t.empty.type:1|\n", b"t.trail:1|ms|\n", b"t.pipe|in.name:1|d\n"]
KIND_STEPS = [2, 2, 2, 2, 2, 127, 127, 2, 2, 127, 127, 127, 2]
KIND_TEXTS = [b"t.c:1|c|@0.2\n", b"t.ms:1|ms|@0.2\n", b"t.h:1|h|@0.2\n", b"t.d:1|d|@0.2\n", b"t.tag:1|ms|@0.2|#a:b,c\n",
              b"t\x00\xff\x80:\x00\xfe|ms|@0.2|#\x00\xff\n", b"t.long:" + b"1" * 1431 + b"|h|@0.2\n",
              b"t.pipe|in.name:1|d|@0.2\n"]


def kinds_batch():
    """Twenty copies of each kind, shuffled, and a last line without a newline; the seed under which the
    restatement keeps at least one line of every sampleable kind."""
    lines = [k for k in KINDS for _ in range(20)]
    order = np.random.default_rng(1).permutation(len(lines))
    lines = [lines[k] for k in order] + [b"t.ms:1|ms"]
    data, recs, hashes = made_up(lines, 2)
    for seed in range(64):
        res = E.apply(data, recs, hashes, 2, 4, E.TYPES_ALL, 0, seed)
        if all(t in res.text for t in KIND_TEXTS):
            return lines, order, seed
    raise AssertionError("no seed keeps a line of every kind")


def test_rewrites_of_every_kind(pkg, torch_stream):
    """Twenty copies of each line under limit 4: step 2, rate 0.2. Every type, tags (the insert stands before `|#`),
    an '@' (untouched), NUL and high bytes, a '|' in the name, the longest line (1441 bytes) and one byte more
    (untouched), and a last line without a newline (untouched)."""
    import torch

    assert len(KINDS[8]) == 1441 and len(KINDS[9]) == 1442
    lines, order, seed = kinds_batch()
    with Dev(pkg, torch, torch_stream, 2, 4, seed=seed) as d:
        for mis in (0, 5):
            res, = d.run([made_up(lines, 2)], f"kinds mis {mis}", mis=(mis, 0, 0))
            got = E.lines_of(b"".join(lines), res.text, res.out)
            assert (res.steps[:-1] & 0x7F).tolist() == [KIND_STEPS[k // 20] for k in order]
            assert int(res.steps[-1]) == E.NOT_SAMPLEABLE and got[-1] == b"t.ms:1|ms"
            assert all(t in got for t in KIND_TEXTS)
            assert all(got.count(KINDS[k]) == 20 for k in (5, 6, 9, 10, 11)) and int(res.out["length"].max()) == 1446


def test_the_longest_rewritten_line_has_1449_bytes(pkg, torch_stream):
    """10,001 lines of one name under limit 1: step 12; among them lines of 1441 bytes, of which a kept one becomes
    1449 bytes with `|@0.0001`. Seed 0 keeps none of the long ones; the seed is chosen so that one is kept."""
    import torch

    long_line = b"one.name:" + b"7" * 1428 + b"|ms\n"
    assert len(long_line) == 1441
    lines = [b"one.name:1|ms\n"] * 9000 + [long_line] * 1001
    data, recs, _ = made_up(lines, 3)
    h = E.name_hash(b"one.name")
    seed = next(s for s in range(1000) if any(E.keep(h, s, i, 12) for i in range(9000, 10001)))
    with Dev(pkg, torch, torch_stream, 3, 1, seed=seed) as d:
        res, = d.run([(data, recs, np.full(len(lines), h, np.uint64))], "1449")
        assert ((res.steps & 0x7F) == 12).all() and int(res.out["length"].max()) == 1449
        assert res.text.count(b"|ms|@0.0001\n") == int(res.counts[2]) >= 1


def test_hostile_and_overlapping_records_pass_through(pkg, torch_stream):
    import torch

    data = b"hot.a:1|ms\nhot.b:22|h\n"
    rng = np.random.default_rng(8)
    recs = np.zeros(700, E.RECORD_DTYPE)
    recs["offset"] = rng.choice([0, 0, 0, 11, 11, 11, 1, 20, 21, 22, 23, 1 << 20, 0xFFFFFFFF, 0xFFFFFFF0], 700)
    recs["length"] = rng.choice([11, 11, 11, 11, 0, 1, 2, 7, 22, 23, 1441, 1449, 0xFFFF], 700)
    recs["route"] = rng.choice([0, 1, 0, 1, 2, 3, 0xFFFC, 0xFFFD, 0xFFFE, 0xFFFF, 77], 700)
    hashes = rng.integers(0, 4, 700).astype(np.uint64)
    with Dev(pkg, torch, torch_stream, 2, 3) as d:
        for mis in (0, 9):
            spec = dict(data=data, recs=recs, hashes=hashes, append_cap=1 << 16)
            res, = d.run([spec], "hostile", mis=(mis, 0, 0))
            ns = res.steps == E.NOT_SAMPLEABLE
            assert 400 < int(ns.sum()) < 690 and int(res.counts[1]) > 10 and int(res.counts[2]) > 3
            assert int(res.counts[3]) > E.append_capacity(len(data))   # overlapping records: the bound does not hold


def test_clamped_device_counts(pkg, torch_stream):
    import torch

    data, recs, hashes = mix(12, 600, 3)
    with Dev(pkg, torch, torch_stream, 3, 2) as d:
        for n_records, max_records in ((1 << 40, 300), (257, 600), (0, 600), (600, 0)):
            spec = dict(data=data, recs=recs, hashes=hashes, n_records=n_records, max_records=max_records)
            res, = d.run([spec], f"n {n_records} max {max_records}")
            assert int(res.counts[0] + res.counts[1]) == min(n_records, max_records)


def test_append_cap_none_short_and_exact(pkg, torch_stream):
    import torch

    data, recs, hashes = E.records_of([b"hot.timer:%d|ms|#t" % i for i in range(700)], 3)
    need = int(E.apply(data, recs, hashes, 3, 200).counts[3])
    assert need > 2000
    with Dev(pkg, torch, torch_stream, 3, 200, types=E.TYPES_DEFAULT) as d:
        for cap in (0, 1, 63, 64, 65, need - 1, need, need + 1):
            res, = d.run([dict(data=data, recs=recs, hashes=hashes, append_cap=cap)], f"cap {cap}", mis=(3, 0, 0))
            assert int(res.counts[3]) == need


def every_length(mis):
    """Sixteen copies of a line of every length 6..80, every other one with tags, shuffled by `mis`."""
    lines = []
    for ln in range(6, 81):
        tail = b"|h|#t" if ln % 2 and ln >= 9 else b"|h"
        line = (b"t" if len(tail) > 2 else b"n") * (ln - 3 - len(tail)) + b":5" + tail + b"\n"
        assert len(line) == ln
        lines += [line] * 16
    return [lines[k] for k in np.random.default_rng(mis).permutation(len(lines))]


@pytest.mark.parametrize("mis", range(16))
def test_every_alignment_and_every_length_of_a_rewritten_line(pkg, torch_stream, mis):
    """Lines of every length 6..80 with sixteen copies each under limit 8 (step 1, `|@0.5`; the insert stands at the
    end or, with tags, in the middle), shuffled, in a batch that begins `mis` bytes past a 16-byte boundary: every
    phase of source and destination occurs, and a rewritten line of every length."""
    import torch

    lines = every_length(mis)
    with Dev(pkg, torch, torch_stream, 2, 8, seed=mis) as d:
        res, = d.run([made_up(lines, 2)], f"mis {mis}", mis=(mis, 4 * (mis & 1), 8 * (mis & 1)))
        assert ((res.steps & 0x7F) == 1).all() and int(res.counts[2]) > 400
        new = res.out[res.out["offset"] >= len(b"".join(lines))]
        assert {int(x) for x in new["length"]} == set(range(6 + 5, 81 + 5))
        assert {(mis + int(x)) % 16 for x in new["offset"]} == set(range(16))


@pytest.mark.parametrize("hashes_out,step", [(False, False), (True, False), (False, True)], ids=["none", "hashes", "step"])
def test_optional_pointers(pkg, torch_stream, hashes_out, step):
    import torch

    with Dev(pkg, torch, torch_stream, 3, 2) as d:
        d.run([mix(20, 515, 3)], "optional", hashes_out=hashes_out, step=step)


def test_32_batches_with_empty_ones_three_calls_then_reset(pkg, torch_stream):
    import torch

    sizes = [0, 1, 255, 256, 257, 0, 513, 3] * 4
    with Dev(pkg, torch, torch_stream, 4, 2, slots=64) as d:
        batches = d.upload([dict(zip(("data", "recs", "hashes", "seed_add"), mix(30 + j, s, 4) + (j,))) for j, s in enumerate(sizes)])
        arr = d.r.sample_batches([b.tuple() for b in batches])
        for _ in range(3):
            d.r.sample(arr)
        res = d.check(batches, "32 batches", calls=3)      # the hits of three calls
        assert sum(int(x.counts[1]) for x in res) > 100
        d.r.sample_reset()
        d.hits[:] = 0
        d.r.sample(arr)
        d.check(batches, "after the reset")


def test_graph_capture_and_replay(pkg, torch_stream):
    import torch

    with Dev(pkg, torch, torch_stream, 3, 2) as d:
        batches = d.upload([mix(50, 700, 3), mix(51, 100, 3)])
        arr = d.r.sample_batches([b.tuple() for b in batches])
        d.r.sample(arr)                                     # sizes the scratch
        d.check(batches, "eager")
        for b in batches:
            for x in b.outputs():
                x.fill()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch_stream):
            d.r.sample(arr)
        g.replay()
        g.replay()
        d.check(batches, "replayed", calls=2)


def test_seeds_pick_the_kept_set(pkg, torch_stream):
    """One batch under seed_add 0, 1 and 0 again: the first and the third keep the same records, the second others."""
    import torch

    data, recs, hashes = E.records_of([b"hot.timer:%d|ms" % i for i in range(800)], 3)
    with Dev(pkg, torch, torch_stream, 3, 8, seed=0xDEADBEEF) as d:
        kept = []
        for add in (0, 1, 0, (1 << 64) - 0xDEADBEEF):
            res, = d.run([dict(data=data, recs=recs, hashes=hashes, seed_add=add)], f"seed_add {add}")
            kept.append((res.steps & E.DROPPED == 0).tolist())
        assert kept[0] == kept[2] and kept[0] != kept[1] and kept[3] != kept[0]
        assert all(2 <= sum(k) <= 30 for k in kept)         # about 800 / 100


def test_argument_errors(pkg, torch_stream):
    import torch

    r = pkg.Router(2, 1 << 16)
    r.set_stream(torch_stream.cuda_stream)
    b, = [DevBatch(torch, dict(zip(("data", "recs", "hashes"), mix(1, 10, 2))))]
    ok = list(b.tuple())

    def rc(t, count=1):
        return pkg.lib().sr_sample(r._h, r.sample_batches([tuple(t)]), count)

    assert rc(ok) == -errno.EINVAL                          # the stage is not open
    for kw in (dict(limit=0), dict(limit=1, types=0), dict(limit=1, types=2), dict(limit=1, types=64), dict(limit=1, slots=8),
               dict(limit=1, slots=48), dict(limit=1, slots=1 << 23), dict(limit=1, reserved=1)):
        with pytest.raises(pkg.SrError) as ei:
            r.sample_open(pkg.SampleConfig(**kw))
        assert ei.value.errno == errno.EINVAL
    with pytest.raises(pkg.SrError):
        r.sample_read()
    with pytest.raises(pkg.SrError):
        r.sample_reset()
    r.sample_open(pkg.SampleConfig(4, slots=1 << 22))
    with pytest.raises(pkg.SrError) as ei:
        r.sample_open(pkg.SampleConfig(4))
    assert ei.value.errno == errno.EBUSY
    assert rc(ok, 0) == -errno.EINVAL and rc(ok, 33) == -errno.EINVAL
    for at in (0, 3, 4, 6, 7, 10):                          # d_bytes, d_recs, d_n_records, d_hashes, d_out, d_counts
        bad = list(ok)
        bad[at] = 0
        assert rc(bad) == -errno.EINVAL, at
    bad = list(ok); bad[7] = ok[3]                          # d_out == d_recs
    assert rc(bad) == -errno.EINVAL
    bad = list(ok); bad[8] = ok[6]                          # d_hashes_out == d_hashes
    assert rc(bad) == -errno.EINVAL
    bad = list(ok); bad[10] = ok[4]                         # d_counts == d_n_records
    assert rc(bad) == -errno.EINVAL
    bad = list(ok); bad[1] = (1 << 30) + 1                  # nbytes
    assert rc(bad) == -errno.EINVAL
    bad = list(ok); bad[1], bad[2] = 1 << 30, 0xFFFFFFF1 - (1 << 30)   # nbytes + append_cap
    assert rc(bad) == -errno.EINVAL
    bad = list(ok); bad[5] = 0xFFFFFFF1                     # max_records
    assert rc(bad) == -errno.EINVAL
    torch.cuda.synchronize()
    b.out.expect(b"", "nothing was launched")
    b.bytes.expect(b.data, "nothing was written")
    assert r.sample_read().sum() == 0 and len(r.sample_read()) == E.STEPS and len(r.sample_read(2)) == 2
    r.sample([tuple(ok)])                                   # and the largest table works
    torch.cuda.synchronize()
    assert int(r.sample_read()[:, 0].sum()) > 0
    r.sample_close()
    r.sample_close()                                        # closing a closed stage is no error
    r.close()


@pytest.mark.parametrize("alive", [[1, 1, 1, 1, 1], [1, 1, 0, 1, 1]], ids=["all-alive", "one-dead"])
def test_route_sample_coalesce_pack_payloads(pkg, torch_stream, alive):
    """The chain on one seeded batch of a few hundred lines: the route launch's records through sr_sample and
    sr_coalesce (which takes the batch and the sample arena as its batch) are the restatements composed in that order
    (records, hashes, counts, both texts); the packing and the payloads of the chain's result equal those of the
    restatement's records, uploaded. A sampled `|c` line is no plain counter any more and is not merged."""
    import torch
    import coalesce_expect as CE

    n = 5
    rng = np.random.default_rng(99)
    pool = POOL[:-1] + [b"hot.counter:1|c", b"hot.counter:3|c", b"hot.other:2|c", b"svc.t:3|ms", b"svc.t:4|ms"]
    lines = [pool[k] for k in rng.integers(0, len(pool), 400)]
    data = b"".join(x + b"\n" for x in lines)
    nb, cap = len(data), len(data)
    arena = E.append_capacity(nb)
    whole = nb + arena + (nb + arena)                       # the batch, the sample arena, the coalesce arena
    mp = pkg.max_packets(whole, n)
    z = lambda k, dt=torch.int64: torch.zeros(max(k, 1), dtype=dt, device="cuda")
    p = lambda t: t.data_ptr()
    with Dev(pkg, torch, torch_stream, n, 6, seed=5) as d:
        r = d.r
        r.set_alive(alive)
        r.coalesce_open(0)
        d_bytes = torch.zeros(whole, dtype=torch.uint8, device="cuda")
        d_bytes[:nb].copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
        d_recs, d_hash, d_sout, d_sh, d_cout = (z(cap) for _ in range(5))
        d_n, d_sc, d_cc = z(1), z(4), z(4)
        d_pd = z((n + 63) // 64)
        r.route_device_many([(p(d_bytes), nb, p(d_recs), cap, p(d_hash), p(d_n), p(d_pd))])
        r.sample([(p(d_bytes), nb, arena, p(d_recs), p(d_n), cap, p(d_hash), p(d_sout), p(d_sh), 0, p(d_sc), 0)])
        r.coalesce([(p(d_bytes), nb + arena, nb + arena, p(d_sout), p(d_sc), cap, p(d_sh), p(d_cout), p(d_cc))])
        torch.cuda.synchronize()
        nrec = int(d_n.cpu().numpy()[0])
        recs = d_recs.cpu().numpy().view(E.RECORD_DTYPE)[:nrec].copy()
        hashes = d_hash.cpu().numpy().view(np.uint64)[:nrec].copy()
        assert nrec == len(lines)
        v = E.apply(data, recs, hashes, n, 6, E.TYPES_ALL, 0, 5)
        ext = data + v.text + bytes(arena - len(v.text))
        w = CE.coalesce(ext, v.out, v.hashes_out, n, CE.DEFAULT_SLOTS, nb + arena)
        assert d_sc.cpu().numpy().view(np.uint64).tolist() == v.counts.tolist()
        assert int(v.counts[1]) > 20 and int(v.counts[2]) > 10 and b"|c|@" in v.text
        assert np.array_equal(d_sout.cpu().numpy().view(E.RECORD_DTYPE)[: len(v.out)], v.out)
        assert np.array_equal(d_sh.cpu().numpy().view(np.uint64)[: len(v.out)], v.hashes_out)
        assert bytes(d_bytes[nb: nb + len(v.text)].cpu().numpy()) == v.text
        assert d_cc.cpu().numpy().view(np.uint64).tolist() == w.counts.tolist()
        assert bytes(d_bytes[2 * nb + arena: 2 * nb + arena + int(w.counts[3])].cpu().numpy()) == w.text
        got_recs = d_cout.cpu().numpy().view(E.RECORD_DTYPE)[: int(w.counts[0])].copy()
        assert np.array_equal(got_recs, w.out)

        def packed(src, cnt):
            d_srt, d_pk, d_counts = z(cap), z(2 * mp), z(4)
            d_fin, d_fout = z(n, torch.int16), z(n, torch.int16)
            r.pack_packets_many([(p(src), p(cnt), cap, p(d_fin), p(d_pd), p(d_srt), p(d_pk), mp, p(d_counts), p(d_fout))])
            pay_cap = whole + 1450 * n
            d_pay, d_off, d_tot = z(pay_cap, torch.uint8), z(mp + 1, torch.int32), z(1)
            r.pack_payloads((p(d_bytes), whole, p(d_srt), cap, p(d_pk), mp, p(d_counts), p(d_fout), 0, 0, p(d_pay), pay_cap,
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
        whole_text = ext + w.text
        for q, pk in enumerate(got[6]):   # (room left for a carry is not written: the bytes of this batch's lines)
            lo = got[4][q] + int(pk[5])
            assert got[7][lo: lo + int(pk[4])] == want[7][lo: lo + int(pk[4])], q
        sent = got[7]
        assert b"|@0." in sent and all(x in whole_text for x in sent.split(b"\n")[:5])
