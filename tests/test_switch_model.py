"""CPU: tests/switch_model.py alone. The GPU switch tests compare a live context with the model bit for bit and
assert no count beyond "> 0" themselves; what keeps them from passing vacuously is checked here: the hostile
traffic really has lines that the rules drop, groups that merge (fewer with 16 slots, so slots do collide), merged
sums <= 0, long names that merge and every kind of invalid line, in every shard state; and the model is the
composition of the restatements it claims to be."""
from __future__ import annotations

import numpy as np
import pytest

import coalesce_expect as CE
import payload_expect as X
import rules_expect as E
import stats_expect as S
import switch_model as M

SEEDS = (1, 2, 3, 4, 5, 7, 8, 9)   # seed 6 has no long name that merges in its batch of 300
STATES = [(6, [1] * 6), (6, [1, 0, 1, 1, 0, 1]), (1, [1])]
IDS = ["6-alive", "6-two-dead", "1-alive"]


def _stages(oracle, data, n, alive, slots):
    recs, hashes, _ = oracle.route(data, n, alive)
    res = E.apply(data, recs, hashes, n, M.RULES)
    co = CE.coalesce(data, res.out, res.hashes_out, n, slots, len(data))
    return recs, res, co


@pytest.mark.parametrize("n,alive", STATES, ids=IDS)
@pytest.mark.parametrize("count", [300, 1500, 3000])
def test_the_traffic_exercises_every_stage(oracle, n, alive, count):
    for seed in SEEDS:
        data = M.hostile_traffic(seed, count)
        assert data.count(b"\n") == count
        recs, res, co = _stages(oracle, data, n, alive, CE.DEFAULT_SLOTS)
        _, _, co16 = _stages(oracle, data, n, alive, 16)
        label = f"seed {seed}"
        assert len(recs) == count, label
        assert int(res.counts[1]) * 4 >= count, (label, res.counts.tolist())          # dropped >= 25 %
        assert int(co.counts[2]) >= 8 and int(co16.counts[2]) >= 5, (label, co.counts.tolist(), co16.counts.tolist())
        assert int(co16.counts[1]) < int(co.counts[1]), (label, co.counts.tolist(), co16.counts.tolist())
        assert co.complete and co16.complete


@pytest.mark.parametrize("n,alive", STATES, ids=IDS)
def test_every_batch_of_300_has_every_kind_of_line(oracle, n, alive):
    for seed in SEEDS:
        data = M.hostile_traffic(seed, 300)
        recs, res, co = _stages(oracle, data, n, alive, CE.DEFAULT_SLOTS)
        label = f"seed {seed}"
        assert (recs["route"] == 0xFFFD).any(), f"{label}: no invalid-length line"
        assert (recs["route"] == 0xFFFE).any(), f"{label}: no line without a colon"
        merged = [CE.parse(l + b"\n") and l for l in co.text.split(b"\n")[:-1]]
        assert merged and all(merged), label
        assert any(CE.parse(l + b"\n")[1] <= 0 for l in merged), f"{label}: no merged sum <= 0"
        assert any(CE.parse(l + b"\n")[0] > 64 for l in merged), f"{label}: no long name that merges"
        kept = [CE.line_of(data, co, r) for r in co.out]
        assert any(l.startswith(b"debug.keep.") for l in kept), f"{label}: no kept debug.keep. line"
        assert not any(l.startswith((b"debug.t", b"host.hot:", b"svc.req.7:", b"\x00\xff")) for l in kept), label


def test_the_matrix_batch_spans_route_tiles_and_cuts_into_datagrams():
    assert M.MATRIX_SEED in SEEDS and M.MATRIX_SEED + 2 in SEEDS   # the matrix's two batches
    data = M.hostile_traffic(M.MATRIX_SEED, 300)
    assert 16384 < len(data) < (1 << 17)           # two 16 KiB route tiles, within the matrix's context
    lines = data.split(b"\n")[:-1]
    assert any(len(l) + 1 >= 1450 for l in lines) and any(l.startswith(b"n" * 1425 + b":") for l in lines)
    dg = M.datagrams(data, M.MATRIX_SEED)
    assert len(dg) > 5 and max(len(d) for d in dg) <= 4095 and not any(d.endswith(b"\n") for d in dg)


def test_datagrams_frame_back_to_the_batch(oracle):
    for data in (b"", b"\n", b"a:1|c\n\n", b"\n\n\nq:1|c\n", M.hostile_traffic(3, 1500)):
        dg = M.datagrams(data, 1)
        assert b"".join(oracle.frame(d) for d in dg) == data
        ends = M.ends_of(dg)
        assert (int(ends[-1]) if len(ends) else 0) == len(data)


# ---- the model's invariants -------------------------------------------------------------------------------------
def test_with_rules_and_coalescing_off_the_model_is_the_payload_expectation(oracle):
    n, alive = 6, [1, 0, 1, 1, 0, 1]
    fills = [0, 7, 1449, 3, 0, 1450]
    for seed, count in ((1, 300), (2, 1), (3, 0), (4, 1500)):
        data = M.hostile_traffic(seed, count)
        m = M.Model(n, 1 << 18)
        m.set_alive(alive)
        m.set_payloads(True)
        x = m.submit(0, data, fills)
        e = X.Expect(oracle, data, n, alive, fills, {k: bytes(f) for k, f in enumerate(fills)})
        assert np.array_equal(x.sorted, e.sorted) and np.array_equal(x.packets, e.packets)
        assert x.fill_out.tolist() == e.fill_out.tolist() and x.n_valid == e.n_valid
        assert x.probed.tolist() == e.probed.tolist()
        assert x.arena == e.arena and np.array_equal(x.offsets, e.offsets) and x.rooms == e.rooms
        assert x.rules_counts is None and x.co_text is None and x.trace is None and x.logtext is None
        assert m.fills == [int(f) for f in e.fill_out]


def test_trace_log_and_statistics_do_not_depend_on_rules_or_coalescing(oracle):
    n, alive = 5, [1, 1, 0, 1, 1]
    batches = [M.hostile_traffic(10 + b, 400) for b in range(3)]
    outs = []
    for rules in (False, True):
        for co in (False, True):
            m = M.Model(n, 1 << 18)
            m.set_alive(alive)
            m.set_trace(True)
            m.set_logtext(M.TRACE, 0, 300)
            m.set_name_stats(True, hll_p=6, cms_rows=3, cms_width=256, hot_slots=16, hot_div=8, hot_min_lines=2)
            m.set_name_rules(M.RULES if rules else None)
            m.set_coalesce(co, 16)
            got = []
            for b, data in enumerate(batches):
                dg = M.datagrams(data, b)
                x = m.submit_slots(b % 2, dg, None, (b"T ", b"W ")) if b == 1 else m.submit(b % 2, data, None, M.ends_of(dg))
                assert (x.rules_counts is not None) == rules and (x.co_counts is not None) == co
                got.append((x.trace, x.logtext))
            outs.append((got, m.stats.read(), m))
    ref = outs[0]
    assert len(ref[0][1][1][0]) > 10000 and ref[1].total > 500 and len(ref[1].hot) > 0
    for got, snap, _ in outs[1:]:
        for (ta, la), (tb, lb) in zip(ref[0], got):
            assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])
            assert la[0] == lb[0] and np.array_equal(la[1], lb[1]) and np.array_equal(la[2], lb[2])
        assert S.same(snap, ref[1]) == []
    # and the packing does depend on them: four different chains
    assert len({tuple(m.fills) for _, _, m in outs}) == 4


def test_the_fill_chain_is_the_oracles_over_the_kept_lines(oracle):
    """A sequence through the model leaves the pending bytes that oracle.pack_packets leaves when it is fed, batch by
    batch, the kept and merged lines as batches of their own."""
    n, alive = 6, [1, 0, 1, 1, 0, 1]
    m = M.Model(n, 1 << 18)
    m.set_alive(alive)
    m.set_name_rules(M.RULES)
    m.set_coalesce(True)
    fills = [5, 0, 1440, 0, 0, 77]
    chain = list(fills)
    for b in range(5):
        data = M.hostile_traffic(20 + b, [300, 0, 1, 900, 300][b])
        x = m.submit(b % 2, data, fills if b == 0 else None)
        recs, res, co = _stages(oracle, data, n, alive, CE.DEFAULT_SLOTS)
        kept = b"".join(CE.line_of(data, co, r) for r in co.out)
        krecs, _, _ = oracle.route(kept, n, alive)
        assert krecs["route"].tolist() == co.out["route"].tolist() and krecs["length"].tolist() == co.out["length"].tolist()
        _, packets, fout, nv = oracle.pack_packets(krecs, n, chain, oracle.probed_dead(data, n, alive))
        assert fout.tolist() == x.fill_out.tolist() and nv == x.n_valid
        assert packets[["nlines", "shard", "length", "carry", "open"]].tolist() == \
            x.packets[["nlines", "shard", "length", "carry", "open"]].tolist()
        chain = fout.tolist()
        assert m.fills == chain
    assert int(m.hits[:, 0].sum()) > 0 and int(m.hits[3, 0]) > 100   # host.hot


def test_the_model_carries_what_the_context_carries():
    m = M.Model(3, 1 << 18)
    data = M.hostile_traffic(5, 300)
    m.set_name_rules(M.RULES)
    m.submit(0, data)
    first = m.hits.copy()
    m.set_name_rules(None)           # off: the hits stay, nothing is added
    assert m.submit(1, data).rules_counts is None and np.array_equal(m.hits, first)
    m.set_name_rules(M.RULES)        # the same set again: a new stage, the hits restart
    assert int(m.hits.sum()) == 0
    m.submit(0, data)
    assert np.array_equal(m.hits, first)
    m.set_name_rules(M.RULES_B)      # a set of another size
    assert m.hits.shape == (len(M.RULES_B) + 1, 2)
    m.set_name_stats(True)
    m.submit(0, data)
    m.set_name_stats(False)          # off and on: the statistics continue
    m.submit(1, data)
    m.set_name_stats(True, hll_p=4)  # (the configuration of the open stage stays)
    m.submit(0, data)
    assert m.stats.read().total == 2 * int((m._route(data)[0]["route"] < 3).sum()) and m.stats.cfg["hll_p"] == 10
    m.set_coalesce(True, 16)
    m.set_coalesce(False)
    m.set_coalesce(True, 64)         # the slot count is fixed once the stage is open
    assert m.co_slots == 16
    m.coalesce_close()
    m.set_coalesce(True)
    assert m.co_slots == CE.DEFAULT_SLOTS


def test_the_matrix_order_is_a_gray_code_over_the_whole_product():
    from test_gpu_switch_matrix import NAMES, combinations

    combos = combinations()
    assert len({(tuple(sorted(c.items())), lv) for c, lv in combos}) == 96
    for (a, la), (b, lb) in zip(combos, combos[1:]):
        assert sum(a[k] != b[k] for k in NAMES) + (la != lb) == 1
    for k in NAMES:   # every switch goes on and off many times
        assert sum(a[k] != b[k] for (a, _), (b, _) in zip(combos, combos[1:])) >= 5
