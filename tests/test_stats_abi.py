"""The name-statistics entry points: declared, listed, exported; the structures the same in C and Python; null
arguments refused before any device use; and the host-only functions (sr_name_hash, sr_stats_estimate,
sr_stats_cardinality, sr_stats_merge) on snapshots built from the restatement. CPU only: needs the built library,
calls no GPU code."""
from __future__ import annotations

import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

import stats_expect as E
from conftest import REPO
from test_abi import _exported, declared_functions

NEW = {"sr_stats_open", "sr_stats_update", "sr_stats_reset", "sr_stats_read", "sr_stats_free", "sr_stats_close",
       "sr_name_hash", "sr_stats_estimate", "sr_stats_cardinality", "sr_stats_merge", "sr_set_name_stats"}
LAYOUTS = {
    "sr_stats_config": ("SrStatsConfig", ("hll_p", "cms_rows", "cms_width", "hot_slots", "hot_div", "hot_min_lines")),
    "sr_stats_batch": ("SrStatsBatch", ("d_bytes", "nbytes", "d_recs", "d_n_records", "max_records", "d_hashes")),
    "sr_stats_hot": ("SrStatsHot", ("hash", "lines", "name_len", "name")),
    "sr_stats_snapshot": ("SrStatsSnapshot", ("cfg", "n_downstreams", "hot_overflow", "lines", "bytes", "ignored",
                                              "shard_lines", "shard_bytes", "regs", "cells", "hot", "n_hot")),
}


def test_new_functions_declared_listed_exported(pkg):
    assert NEW <= declared_functions()
    assert NEW <= set(pkg.ABI_FUNCTIONS)
    assert NEW <= _exported(pkg.ROUTE_LIB)
    lib = pkg.lib()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name
    for name in ("stats_open", "stats_update", "stats_reset", "stats_read", "stats_close", "set_name_stats"):
        assert callable(getattr(pkg.Router, name)), name


def test_structures_and_macros_match_c(pkg, tmp_path):
    body = []
    for cname, (_, fields) in LAYOUTS.items():
        body.append(f'printf("%zu", sizeof({cname}));')
        body += [f'printf(" %zu", offsetof({cname}, {f}));' for f in fields]
        body.append('printf("\\n");')
    macros = ("SR_STATS_NAME_MAX", "SR_STATS_ALL", "SR_STATS_MIN_P", "SR_STATS_MAX_P", "SR_STATS_MAX_REGS",
              "SR_STATS_MAX_ROWS", "SR_STATS_MIN_WIDTH", "SR_STATS_MAX_CELLS", "SR_STATS_MIN_SLOTS", "SR_STATS_MAX_SLOTS",
              "SR_STATS_DEFAULT_P", "SR_STATS_DEFAULT_ROWS", "SR_STATS_DEFAULT_WIDTH", "SR_STATS_DEFAULT_SLOTS",
              "SR_STATS_DEFAULT_HOT_DIV", "SR_STATS_DEFAULT_HOT_MIN")
    body += [f'printf("%llu ", (unsigned long long){m});' for m in macros]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sr_route.h"\nint main(void) { %s return 0; }\n'
                   % " ".join(body))
    exe = tmp_path / "sizes"
    subprocess.run([os.environ.get("CC", "cc"), "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    rows = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    for row, (cname, (pyname, fields)) in zip(rows, LAYOUTS.items()):
        nums = list(map(int, row.split()))
        cls = getattr(pkg, pyname)
        assert ctypes.sizeof(cls) == nums[0], cname
        assert [getattr(cls, f).offset for f in fields] == nums[1:], cname
    assert ctypes.sizeof(pkg.SrStatsHot) == 128 == pkg.STATS_HOT_DTYPE.itemsize == E.HOT_DTYPE.itemsize
    vals = dict(zip(macros, map(int, rows[len(LAYOUTS)].split())))
    assert vals["SR_STATS_NAME_MAX"] == pkg.SR_STATS_NAME_MAX == E.NAME_MAX == 108
    assert vals["SR_STATS_ALL"] == pkg.SR_STATS_ALL == E.ALL
    assert vals["SR_STATS_MAX_CELLS"] == pkg.SR_STATS_MAX_CELLS == 16384
    assert (vals["SR_STATS_MIN_P"], vals["SR_STATS_MAX_P"], vals["SR_STATS_MAX_REGS"]) == (4, 12, 1 << 26)
    assert (vals["SR_STATS_MAX_ROWS"], vals["SR_STATS_MIN_WIDTH"]) == (8, 256)
    assert (vals["SR_STATS_MIN_SLOTS"], vals["SR_STATS_MAX_SLOTS"]) == (4, 4096)
    defaults = dict(hll_p=vals["SR_STATS_DEFAULT_P"], cms_rows=vals["SR_STATS_DEFAULT_ROWS"],
                    cms_width=vals["SR_STATS_DEFAULT_WIDTH"], hot_slots=vals["SR_STATS_DEFAULT_SLOTS"],
                    hot_div=vals["SR_STATS_DEFAULT_HOT_DIV"], hot_min_lines=vals["SR_STATS_DEFAULT_HOT_MIN"])
    assert defaults == pkg.SR_STATS_DEFAULTS == E.DEFAULTS


def test_null_arguments_are_refused_without_a_device(pkg):
    lib, inval = pkg.lib(), -errno.EINVAL
    cfg, batch = pkg.SrStatsConfig(), pkg.SrStatsBatch()
    assert lib.sr_stats_open(None, None) == inval
    assert lib.sr_stats_open(None, ctypes.byref(cfg)) == inval
    assert lib.sr_stats_update(None, None, 1) == inval
    assert lib.sr_stats_update(None, ctypes.byref(batch), 1) == inval
    assert lib.sr_stats_reset(None) == inval
    assert lib.sr_stats_close(None) == inval
    p = ctypes.POINTER(pkg.SrStatsSnapshot)()
    assert lib.sr_stats_read(None, ctypes.byref(p)) == inval and not p
    assert lib.sr_stats_read(None, None) == inval
    assert lib.sr_set_name_stats(None, None) == inval
    assert lib.sr_set_name_stats(None, ctypes.byref(cfg)) == inval
    lib.sr_stats_free(None)
    assert lib.sr_stats_merge(None, None) == inval
    assert lib.sr_stats_estimate(None, 5) == 0
    assert lib.sr_stats_cardinality(None, 0) < 0


CFG = dict(hll_p=8, cms_rows=3, cms_width=512, hot_slots=8, hot_div=8, hot_min_lines=4)


def _session(seed, n=5, cfg=CFG, names=400):
    rng = np.random.default_rng(seed)
    lines = [b"svc%d.req.%d:1|c" % (seed, int(i)) for i in rng.integers(0, names, 1500)]
    lines += [b"hot.%d:1|c" % (seed % 2)] * 700 + [b"both:2|c"] * 500 + [b"x" * 3, b"no colon here"]
    st = E.Stats(n, cfg)
    st.update([E.records_of(lines, n)])
    return st.read()


def test_host_functions_on_restated_snapshots(pkg):
    snap = _session(1)
    c = E.to_pkg(pkg, snap)
    assert len(snap.hot) >= 2
    for h in [int(x) for x in snap.hot["hash"]] + [0, 1, E.name_hash(b"svc1.req.7"), (1 << 64) - 1]:
        assert pkg.stats_estimate(c, h) == E.estimate(snap, h)
    for shard in list(range(snap.n)) + [E.ALL]:
        want = E.cardinality(snap, shard)
        assert pkg.stats_cardinality(c, shard) == pytest.approx(want, rel=1e-12)
    assert pkg.stats_cardinality(c, snap.n) < 0   # no such shard


@pytest.mark.parametrize("p", [4, 5, 6, 7, 12])
def test_cardinality_alpha_and_small_range(pkg, p):
    """m = 16, 32, 64 have their own alpha; few names stay in linear counting, many leave it."""
    cfg = dict(CFG, hll_p=p, hot_min_lines=1 << 30)
    for count in (3, 40, 5000):
        st = E.Stats(2, cfg)
        st.update([E.records_of([b"name.%d:1|c" % i for i in range(count)], 2)])
        snap = st.read()
        for shard in (0, 1, E.ALL):
            assert pkg.stats_cardinality(E.to_pkg(pkg, snap), shard) == pytest.approx(E.cardinality(snap, shard), rel=1e-12)


def test_merge_matches_the_restatement(pkg):
    a, b = _session(1), _session(2)
    ca, cb = E.to_pkg(pkg, a), E.to_pkg(pkg, b)
    pkg.stats_merge(ca, cb)
    E.merge(a, b)
    assert E.same(ca, a) == []
    assert {bytes(e["name"][: e["name_len"]]) for e in a.hot} >= {b"hot.0", b"hot.1", b"both"}
    assert E.estimate(a, E.name_hash(b"both")) >= 1000
    assert E.same(cb, _session(2)) == []   # `from` is not written


def test_merge_overflow_and_mismatch(pkg):
    small = dict(CFG, hot_slots=4, hot_div=1000, hot_min_lines=100)

    def four(tag):
        st = E.Stats(3, small)
        st.update([E.records_of([b"%s%d:1|c" % (tag, i) for i in range(4) for _ in range(150)], 3)])
        return st.read()

    a, b = four(b"left"), four(b"right")
    assert len(a.hot) == 4 == len(b.hot) and not a.hot_overflow
    ca, cb = E.to_pkg(pkg, a), E.to_pkg(pkg, b)
    pkg.stats_merge(ca, cb)
    E.merge(a, b)
    assert a.hot_overflow == 1 and E.same(ca, a) == []
    assert len(set(ca.hot["hash"].tolist())) == 4
    lib = pkg.lib()
    other = E.to_pkg(pkg, _session(3, cfg=dict(CFG, cms_width=256)))
    base = E.to_pkg(pkg, _session(3))
    assert lib.sr_stats_merge(ctypes.byref(base.sync_c()), ctypes.byref(other.sync_c())) == -errno.EINVAL
    fewer = E.to_pkg(pkg, _session(3, n=4))
    assert lib.sr_stats_merge(ctypes.byref(base.sync_c()), ctypes.byref(fewer.sync_c())) == -errno.EINVAL
    assert E.same(base, _session(3)) == []
