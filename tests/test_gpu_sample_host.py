"""GPU: sr_set_sample, the sample rates of the host-memory path. Double-buffered, slot and synchronous submissions
with payloads and trace, in all sixteen combinations of this switch with the line grammar, the name rules and the
coalescing, against tests/sample_switch_model.py: `sorted`, `packets`, `fill` and the payloads are the oracle's packing
of the restatements composed in the order route, validate, rules, sample, coalesce; the rewritten text, the counts
and the seed come back through sr_route_pack_sample; seed_add advances per accepted submission; the trace, the log
text and the name statistics are those of the switch off; a toggle with a slot in flight is -EBUSY."""
from __future__ import annotations

import errno

import numpy as np
import pytest

import sample_expect as E
import validate_expect as VE
from sample_switch_model import Model
from test_gpu_rules_host import RULES

pytestmark = pytest.mark.gpu

DROP = (1 << VE.VALUE) | (1 << VE.TYPE) | (1 << VE.NO_TYPE) | (1 << VE.RATE) | (1 << VE.TAGS) | (1 << VE.SECTION)
LIMIT, SEED = 6, 0xFFFFFFFFFFFFFFFE   # the seed wraps at the third submission


def traffic(seed, count):
    rng = np.random.default_rng(seed)
    kinds = [b"host.hot:1|c", b"host.hot:2|c", b"debug.t%d:%d|c", b"svc.req.%d:%d|c", b"svc.lat.%d:%d|ms|@0.5", b"svc.g.%d:+%d|g",
             b"svc.bad.%d:x%d|c", b"svc.time:%d.%d|ms", b"svc.time:%d%d|ms|#env:prod", b"svc.hist:%d%d|h", b"svc.dist.%d:%d|d",
             b"debug.time:%d%d|ms", b"svc.nt.%d:%d", b"bad", b"no colon in this line", b"svc.req.7:1|c|#a:b"]
    lines = []
    for k, a, v in zip(rng.integers(0, len(kinds), count), rng.integers(0, 9, count), rng.integers(1, 500, count)):
        f = kinds[k]
        lines.append(f % (a, v) if b"%d" in f else f)
    return b"".join(l + b"\n" for l in lines)


def check(r, slot, w, label, seed):
    from test_gpu_mtu import assert_pack_equal
    from test_gpu_payloads import _check_host

    assert_pack_equal(r.route_pack_result(slot), w.pack())
    if w.v is not None:
        assert r.route_pack_validate(slot).tolist() == w.v.counts.tolist(), label
    if w.res is not None:
        assert r.route_pack_rules(slot).tolist() == w.res.counts.tolist(), label
    if w.sa is not None:
        text, counts, got_seed = r.route_pack_sample(slot)
        assert text == w.sa.text and counts.tolist() == w.sa.counts.tolist() and got_seed == seed & E.M64, label
    if w.co is not None:
        text, counts = r.route_pack_coalesced(slot)
        assert text == w.co.text and counts.tolist() == w.co.counts.tolist(), label
    _check_host(r.route_pack_payloads(slot), w, label)
    recs, hs = r.route_pack_trace(slot)
    assert np.array_equal(recs, w.recs) and np.array_equal(hs, w.hashes), f"{label}: trace"


def test_sixteen_switch_combinations_on_three_paths(pkg, oracle):
    """One context; for each of the sixteen combinations the three submit paths in turn (48 submissions)."""
    import frame_slots as F

    n = 5
    rng = np.random.default_rng(17)
    hits = np.zeros((E.STEPS, 2), np.uint64)
    with pkg.Router(n, 1 << 18) as r:
        r.route_pack_submit(0, b"k:1|c\nk:2|c\n")
        r.route_pack_result(0)
        with pytest.raises(pkg.SrError) as ei:   # submitted with the switch off
            r.route_pack_sample(0)
        assert ei.value.errno == errno.EBUSY
        with pytest.raises(pkg.SrError) as ei:   # a bad configuration leaves the switch off
            r.set_sample(pkg.SampleConfig(0))
        assert ei.value.errno == errno.EINVAL
        r.set_trace(True)
        r.set_payloads(True)
        fill = [0] * n
        k = subs = sampled_counters = 0
        sample_on = False
        for combo in range(16):
            validate, rules, sample, coalesce = (bool(combo >> b & 1) for b in (0, 1, 2, 3))
            r.set_validate(pkg.ValidateConfig(DROP) if validate else None)
            r.set_name_rules(pkg.RuleSet(RULES) if rules else None)
            r.set_coalesce(coalesce)
            if sample and not sample_on:   # switched on: the stage is opened again and seed_add starts at 0
                r.set_sample(pkg.SampleConfig(LIMIT, E.TYPES_ALL, 0, SEED))
                subs = 0
                hits[:] = 0
            elif not sample and sample_on:
                r.set_sample(None)
            sample_on = sample
            for path in ("submit", "slots", "batch"):
                k += 1
                label = f"{path} validate={validate} rules={rules} sample={sample} coalesce={coalesce}"
                alive = (rng.random(n) > 0.25).astype(int).tolist() if k % 3 == 0 else None
                r.set_alive(alive if alive is not None else [1] * n)
                seed = SEED + subs
                kw = dict(validate=DROP if validate else None, rules=RULES if rules else None, coalesce=coalesce,
                          sample=dict(limit=LIMIT, types=E.TYPES_ALL, seed=seed) if sample else None)
                if path == "slots":
                    dgrams = [traffic(500 + 40 * k + i, int(rng.integers(1, 30)))[:-1] for i in range(60)]
                    data = b"".join(d + b"\n" for d in dgrams)
                    arena, lens = F.build_arena(dgrams, 4096)
                    buf = pkg.HostBuffer(arena.size)
                    buf.array[:] = arena
                    r.route_pack_submit_slots(k % 2, buf, 4096, lens, fill)
                    with pytest.raises(pkg.SrError) as ei:   # a toggle with a slot in flight
                        r.set_sample(None)
                    assert ei.value.errno == errno.EBUSY
                    w = Model(oracle, data, n, alive, fill, **kw)
                    check(r, k % 2, w, label, seed)
                elif path == "submit":
                    data = traffic(100 + k, int(rng.integers(300, 900)))
                    r.route_pack_submit(k % 2, data, fill)
                    if sample:
                        with pytest.raises(pkg.SrError) as ei:
                            r.route_pack_sample(k % 2)
                        assert ei.value.errno == errno.EBUSY
                    w = Model(oracle, data, n, alive, fill, **kw)
                    check(r, k % 2, w, label, seed)
                else:
                    data = traffic(100 + k, int(rng.integers(300, 900)))
                    w = Model(oracle, data, n, alive, fill, **kw)
                    srt, pk, fo, nv, pr = r.route_pack(data, fill)
                    assert np.array_equal(srt, w.sorted) and np.array_equal(pk.view(np.uint8), w.packets.view(np.uint8)), label
                    assert nv == w.n_valid and [int(f) for f in fo] == [int(f) for f in w.fill_out], label
                    if sample:
                        text, counts, got_seed = r.route_pack_sample(2)
                        assert text == w.sa.text and counts.tolist() == w.sa.counts.tolist() and got_seed == seed & E.M64, label
                if sample:
                    subs += 1
                    hits += w.sa.hits
                    assert int(w.sa.counts[1]) > 10 and int(w.sa.counts[2]) > 3, label
                    sampled_counters += coalesce and b"|c|@" in w.sa.text   # which the coalescing leaves alone
                fill = [int(f) for f in w.fill_out]
            if sample:
                assert r.sample_read().tolist() == hits.tolist()
        assert k == 48 and sampled_counters >= 6
        r.sample_close()                                   # the switch goes with the stage
        r.set_validate(None)
        r.set_name_rules(None)
        r.set_coalesce(False)
        r.route_pack_submit(0, b"a.b:1|ms\na.b:2|ms\n")
        assert len(r.route_pack_result(0)[0]) == 2


def test_seed_add_counts_the_accepted_submissions(pkg, oracle):
    """One batch five times: the kept sets are those of the seeds cfg.seed, + 1, ... (an empty submission counts, a
    refused one does not), and setting the switch again starts at cfg.seed."""
    n = 3
    data = b"".join(b"hot.timer:%d|ms\n" % i for i in range(600))
    with pkg.Router(n, 1 << 16) as r:
        cfg = pkg.SampleConfig(8, seed=41)
        r.set_sample(cfg)
        seen = []
        for b, payload in enumerate((data, data, b"", data, data)):
            if b == 3:
                with pytest.raises(pkg.SrError):           # no final newline: refused, not counted
                    r.route_pack_submit(b % 2, data[:-1])
            r.route_pack_submit(b % 2, payload, [0] * n)
            srt = r.route_pack_result(b % 2)[0]
            text, counts, seed = r.route_pack_sample(b % 2)
            assert seed == 41 + b
            if payload:
                w = Model(oracle, data, n, None, [0] * n, sample=dict(limit=8, seed=41 + b))
                assert text == w.sa.text and np.array_equal(srt, w.sorted) and counts.tolist() == w.sa.counts.tolist()
                seen.append(text)
            else:
                assert text == b"" and counts.tolist() == [0, 0, 0, 0]
        assert len(set(seen)) == 4
        r.set_sample(cfg)
        r.route_pack_submit(0, data, [0] * n)
        r.route_pack_result(0)
        assert r.route_pack_sample(0)[0] == seen[0] and r.route_pack_sample(0)[2] == 41


def test_logs_trace_and_statistics_are_those_of_the_switch_off(pkg):
    """The log text at TRACE level, the trace and the name statistics, byte for byte, with the switch off and on."""
    n = 5
    outs = []
    for on in (False, True):
        with pkg.Router(n, 1 << 17) as r:
            r.set_logtext(pkg.SR_LOG_TRACE)
            r.set_name_stats(True, hll_p=6, cms_rows=3, cms_width=256, hot_slots=16, hot_div=8, hot_min_lines=2)
            r.set_trace(True)
            if on:
                r.set_sample(pkg.SampleConfig(4, E.TYPES_ALL))
            got = []
            for b in range(3):
                r.route_pack_set_prefix(b % 2, b"T%d " % b, b"W%d " % b)
                r.route_pack_submit(b % 2, traffic(70 + b, 1200), [0] * n if b == 0 else None)
                r.route_pack_result(b % 2)
                got.append((r.route_pack_logtext(b % 2), r.route_pack_trace(b % 2)))
            if on:
                assert int(r.route_pack_sample(0)[1][1]) > 100
            outs.append((got, r.stats_read()))
    for (la, ta), (lb, tb) in zip(outs[0][0], outs[1][0]):
        assert la[0] == lb[0] and la[1] == lb[1] and np.array_equal(la[2], lb[2]) and np.array_equal(la[3], lb[3])
        assert len(la[0]) > 1000
        assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])
    a, b = outs[0][1], outs[1][1]
    assert np.array_equal(a.lines, b.lines) and np.array_equal(a.cells, b.cells) and np.array_equal(a.regs, b.regs)
    assert np.array_equal(a.hot, b.hot) and a.n_hot > 0


def test_the_buffer_limit(pkg):
    """A context whose batches may pass 2^30 bytes cannot sample: -EINVAL before anything is allocated, and the
    switch stays off."""
    with pkg.Router(2, (1 << 30) + 4096) as r:
        with pytest.raises(pkg.SrError) as ei:
            r.set_sample(pkg.SampleConfig(4))
        assert ei.value.errno == errno.EINVAL
        with pytest.raises(pkg.SrError):
            r.sample_read()                                # the stage was not opened
