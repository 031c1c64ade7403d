"""The packet-payload entry points (sr_pack_payloads*, sr_set_payloads, sr_route_pack_payloads,
sr_core_set_payloads): declared, listed, exported, the structure and constants the same in C and
Python, and SR_PAYLOAD_CAPACITY an upper bound of what the oracle's descriptors need. CPU only: needs
the built libraries, calls no GPU code."""
from __future__ import annotations

import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import byte_streams as B
import payload_expect as X
from conftest import REPO
from test_abi import _exported, declared_functions

NEW_ROUTE = {"sr_pack_payloads_many", "sr_pack_payloads", "sr_set_payloads", "sr_route_pack_payloads"}


def test_new_functions_declared_listed_exported(pkg):
    assert NEW_ROUTE <= declared_functions()
    assert NEW_ROUTE <= set(pkg.ABI_FUNCTIONS)
    assert NEW_ROUTE <= _exported(pkg.ROUTE_LIB)
    lib = pkg.lib()
    for name in NEW_ROUTE:
        assert getattr(lib, name).argtypes is not None, name
    core = importlib.import_module("statsd-router_amd.core")
    core.router_lib()
    assert "sr_core_set_payloads" in declared_functions("sr_router.h")
    assert "sr_core_set_payloads" in _exported(core.ROUTER_LIB)
    for name in ("set_payloads", "route_pack_payloads", "pack_payloads", "pack_payloads_many"):
        assert callable(getattr(pkg.Router, name)), name
    assert callable(core.Core.set_payloads)


def test_constants_and_structure_match_c(pkg, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "sr_route.h"\n'
                   'int main(void) { printf("%zu %u %llu %zu %zu\\n", sizeof(sr_payload_batch), SR_PENDING_STRIDE, '
                   '(unsigned long long)SR_PAYLOAD_CAPACITY(1000003, 77), offsetof(sr_payload_batch, d_pend_out), '
                   'offsetof(sr_payload_batch, d_total)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run([os.environ.get("CC", "cc"), "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    size, stride, capv, o_pout, o_total = map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                                                  check=True).stdout.split())
    assert ctypes.sizeof(pkg.SrPayloadBatch) == size
    assert pkg.SrPayloadBatch.d_pend_out.offset == o_pout and pkg.SrPayloadBatch.d_total.offset == o_total
    assert pkg.PENDING_STRIDE == stride == X.STRIDE
    assert stride % 16 == 0 and stride >= pkg.SR_DOWNSTREAM_BUF_SIZE
    assert pkg.payload_capacity(1000003, 77) == capv == 1000003 + 1450 * 77


def _need(oracle, data, n, alive, fills):
    rng = np.random.default_rng(1)
    e = X.Expect(oracle, data, n, alive, fills, X.random_pending(rng, fills))
    assert len(e.arena) == e.total == int(e.packets["carry"].astype(np.int64).sum() + e.packets["length"].astype(np.int64).sum())
    return e.total


def test_capacity_bounds_the_ragged_stream(pkg, oracle):
    data = B.ragged_stream(1, 3 << 20)
    for n in (1, 7, 64):
        for fills in ([0] * n, [1450] * n, [1] * n):
            assert _need(oracle, data, n, None, fills) <= pkg.payload_capacity(data.size, n)


def test_capacity_bounds_seeded_draws(pkg, oracle):
    """200 seeded (n, fills) draws over cuts of a mixed stream, some downstreams dead."""
    rng = np.random.default_rng(0xCAFE)
    stream = pkg.gen_stream(1 << 18, [6, 64, 300, 1449], seed=0x9A1, p_invalid=0.05).data
    worst = 0.0
    for _ in range(200):
        n = int(rng.choice([1, 2, 3, 7, 16, 64, 300]))
        fills = rng.integers(0, 1451, n).tolist() if rng.random() < 0.7 else [1450] * n
        alive = (rng.random(n) > 0.25).astype(int).tolist() if rng.random() < 0.5 else None
        data = B.cut_at_newline(stream, 0, int(rng.integers(1500, stream.size)))
        need = _need(oracle, data, n, alive, fills)
        assert need <= pkg.payload_capacity(data.size, n), (n, data.size, need)
        worst = max(worst, need / pkg.payload_capacity(data.size, n))
    assert worst > 0.5   # the draws do press on the bound
