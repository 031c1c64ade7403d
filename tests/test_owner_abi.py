"""The owner-side entry points (sr_exchange_dead_run, sr_exchange_dead, sr_owner_pack, sr_flush_pending):
declared, listed, exported, sr_owner_batch the same in C and Python, argument errors answered before any
device is touched, and the helper module's expectations consistent with the oracle. CPU only: needs the
built libraries, calls no GPU code."""
from __future__ import annotations

import ctypes
import errno
import importlib
import os
import subprocess

import numpy as np

import owner_expect as O
import payload_expect as X
from conftest import REPO
from test_abi import _exported, declared_functions

NEW = {"sr_exchange_dead_run", "sr_exchange_dead", "sr_owner_pack", "sr_flush_pending"}


def test_new_functions_declared_listed_exported(pkg):
    assert NEW <= declared_functions()
    assert NEW <= set(pkg.ABI_FUNCTIONS)
    assert NEW <= _exported(pkg.ROUTE_LIB)
    lib = pkg.lib()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name
    for name in ("exchange_dead_run", "exchange_dead", "owner_pack", "flush_pending"):
        assert callable(getattr(pkg.Router, name)), name
    rg = importlib.import_module("statsd-router_amd.regroup")
    assert callable(rg.OwnerPacker)


def test_owner_batch_matches_c(pkg, tmp_path):
    names = [f for f, _ in pkg.SrOwnerBatch._fields_]
    src = tmp_path / "owner.c"
    src.write_text('#include <stdio.h>\n#include "sr_route.h"\nint main(void) {\n'
                   '  printf("%zu %u", sizeof(sr_owner_batch), SR_MAX_OWNERS);\n'
                   + "".join(f'  printf(" %zu", offsetof(sr_owner_batch, {f}));\n' for f in names)
                   + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "owner"
    subprocess.run([os.environ.get("CC", "cc"), "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert ctypes.sizeof(pkg.SrOwnerBatch) == out[0]
    assert pkg.SR_MAX_OWNERS == out[1]
    assert [getattr(pkg.SrOwnerBatch, f).offset for f in names] == out[2:]


def test_argument_errors_need_no_device(pkg):
    """Every argument check of sr_exchange_dead_run comes before the context is used: a context that is
    only zeroed memory is never read when another argument is wrong."""
    lib = pkg.lib()
    fake = ctypes.create_string_buffer(1 << 16)   # stands in for a context; must not be dereferenced
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    err = []
    t = pkg._transport_struct(pkg.Transport(), err)
    rows = np.zeros(64 * 64, dtype=np.uint64)
    batches = (pkg.SrBatch * 33)()
    run = lambda c, tr, world, rank, b, count, dead: lib.sr_exchange_dead_run(c, tr, world, rank, b, count, dead)
    ok = (ctx, ctypes.byref(t), 2, 0, batches, 2, rows.ctypes.data)
    for i, bad in [(0, None), (1, None), (2, 0), (2, 65), (2, -1), (3, -1), (3, 2), (4, None), (5, 33), (6, None)]:
        args = list(ok)
        args[i] = bad
        assert run(*args) == -errno.EINVAL, (i, bad)
    # several ranks need the transport's group, send and recv callbacks
    null_fn = pkg.SrTransport()
    assert run(ctx, ctypes.byref(null_fn), 2, 1, batches, 1, rows.ctypes.data) == -errno.EINVAL
    assert lib.sr_exchange_dead(None, None, batches, 1, rows.ctypes.data) == -errno.EINVAL
    assert lib.sr_exchange_dead(ctx, None, batches, 1, rows.ctypes.data) == -errno.EINVAL
    assert lib.sr_owner_pack(None, ctypes.byref(pkg.SrOwnerBatch())) == -errno.EINVAL
    assert lib.sr_owner_pack(ctx, None) == -errno.EINVAL
    for world in (0, 65):   # (checked before the context is read)
        assert lib.sr_owner_pack(ctx, ctypes.byref(pkg.SrOwnerBatch(d_recv_counts=rows.ctypes.data, world=world))) \
            == -errno.EINVAL
    assert lib.sr_flush_pending(None, None, None, None, 0, None, None, 0, None, None) == -errno.EINVAL
    assert not err


def test_expectation_is_the_issue_s_serial_order(pkg, oracle):
    """The helper's owner expectation on a two-source stream: a shard one source probed dead and the other
    sent lines to loses its old pending bytes and keeps the lines, which the packing's own bitmap rule
    (flagged shard: fill_out = 0) would lose."""
    n, k = 4, 2
    line = b"owner.metric.%d:1|c\n"
    lines = [line % i for i in range(40)]
    to_k = [l for l in lines if int(oracle.route(np.frombuffer(l, np.uint8), n)[0]["route"][0]) == k]
    assert len(to_k) >= 2
    data = np.frombuffer(b"".join(to_k), dtype=np.uint8)
    recs = oracle.route(data, n)[0]
    fills = [100, 200, 300, 400]
    pending = X.random_pending(np.random.default_rng(3), fills)
    e = O.OwnerExpect(oracle, n, data, recs, {k}, fills, pending)
    assert int(e.packets[0]["carry"]) == 0 and int(e.packets[0]["shard"]) == k
    assert int(e.fill_out[k]) == data.size and e.new_pending[k] == data.tobytes()
    assert [int(e.fill_out[s]) for s in (0, 1, 3)] == [100, 200, 400]
    _, _, wrong_fill, _ = oracle.pack_packets(recs, n, fills, (k,))
    assert int(wrong_fill[k]) == 0   # the one-GPU rule: the lines would be gone
    f = O.FlushExpect(pkg, n, e.fill_out, e.new_pending, max_packets=n, payload_cap=1 << 20)
    assert f.needed == 4 and f.total == 700 + data.size and not f.fill_after.any()
    assert f.arena == b"".join(e.new_pending[s] for s in range(n))
