"""The coalescing entry points (sr_coalesce_open, sr_coalesce_close, sr_coalesce, sr_coalesce_parse,
sr_coalesce_format): declared, listed, exported, the structures and constants the same in C and Python, argument
errors that need no device, and the two host functions against tests/coalesce_expect.py. CPU only: needs the
built libraries, calls no GPU code."""
from __future__ import annotations

import ctypes
import errno
import os
import re
import subprocess

import numpy as np
import pytest

import coalesce_expect as E
from conftest import REPO
from test_abi import _exported, declared_functions
from test_coalesce_expect import ACCEPTED, REJECTED

NEW = {"sr_coalesce_open", "sr_coalesce_close", "sr_coalesce", "sr_coalesce_parse", "sr_coalesce_format"}


def test_new_functions_declared_listed_exported(pkg):
    assert NEW <= declared_functions()
    assert NEW <= set(pkg.ABI_FUNCTIONS)
    assert NEW <= _exported(pkg.ROUTE_LIB)
    lib = pkg.lib()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name
    for name in ("coalesce_open", "coalesce_close", "coalesce", "coalesce_batches"):
        assert callable(getattr(pkg.Router, name)), name


def test_structures_and_constants_match_c(pkg, tmp_path):
    names = [f for f, _ in pkg.SrCoalesceBatch._fields_]
    consts = ["SR_COALESCE_NAME_MAX", "SR_COALESCE_MIN_SLOTS", "SR_COALESCE_MAX_SLOTS", "SR_COALESCE_DEFAULT_SLOTS",
              "SR_COALESCE_MAX_BYTES"]
    src = tmp_path / "coalesce.c"
    src.write_text('#include <stdio.h>\n#include "sr_route.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu", sizeof(sr_coalesce_batch), sizeof(sr_coalesce_config),'
                   ' (size_t)SR_COALESCE_APPEND_CAPACITY(12345u));\n'
                   + "".join(f'  printf(" %zu", offsetof(sr_coalesce_batch, {f}));\n' for f in names)
                   + "".join(f'  printf(" %lu", (unsigned long){c});\n' for c in consts)
                   + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "coalesce"
    subprocess.run([os.environ.get("CC", "cc"), "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert ctypes.sizeof(pkg.SrCoalesceBatch) == out[0] and ctypes.sizeof(pkg.SrCoalesceConfig) == out[1]
    assert pkg.coalesce_append_capacity(12345) == out[2] == E.append_capacity(12345)
    assert [getattr(pkg.SrCoalesceBatch, f).offset for f in names] == out[3:3 + len(names)]
    assert [getattr(pkg, c) for c in consts] == out[3 + len(names):]
    assert (E.NAME_MAX, E.MIN_SLOTS, E.MAX_SLOTS, E.DEFAULT_SLOTS, E.MAX_BYTES) == tuple(out[3 + len(names):])


def test_tile_constant_is_the_kernels(pkg):
    src = open(os.path.join(REPO, "statsd-router_amd", "csrc", "coalesce_kernel.hpp")).read()
    block = int(re.search(r"constexpr int kCoalesceBlock = (\d+);", src).group(1))
    assert re.search(r"constexpr int kCoalesceTile = kCoalesceBlock;", src)
    assert pkg.COALESCE_TILE == block


def test_argument_errors_need_no_device(pkg):
    lib = pkg.lib()
    b = (pkg.SrCoalesceBatch * 1)()
    assert lib.sr_coalesce_open(None, ctypes.byref(pkg.SrCoalesceConfig(0))) == -errno.EINVAL
    assert lib.sr_coalesce_open(None, None) == -errno.EINVAL
    assert lib.sr_coalesce_close(None) == -errno.EINVAL
    assert lib.sr_coalesce(None, b, 1) == -errno.EINVAL
    assert lib.sr_coalesce_parse(None, 6, None, None) == 0
    assert lib.sr_coalesce_format(None, None, 0, 1) == 0


@pytest.mark.parametrize("line,k,v", ACCEPTED, ids=[str(i) for i in range(len(ACCEPTED))])
def test_parse_accepts(pkg, line, k, v):
    assert pkg.coalesce_parse(line) == (k, v) == E.parse(line)
    buf = (ctypes.c_uint8 * len(line)).from_buffer_copy(line)
    assert pkg.lib().sr_coalesce_parse(buf, len(line), None, None) == 1   # the outputs are optional


@pytest.mark.parametrize("line", REJECTED, ids=[str(i) for i in range(len(REJECTED))])
def test_parse_rejects(pkg, line):
    assert pkg.coalesce_parse(line) is None


def test_parse_agrees_with_the_restatement_on_mutations(pkg):
    """Every single-byte change, deletion and insertion of a few plain counters, from a small alphabet."""
    rng = np.random.default_rng(5)
    alphabet = b":|c\n-+.0123456789 \r@#ax\x00\xff"
    seeds = [b"a:1|c\n", b"ab.c:-12|c\n", b"x:999999999|c\n", b"q:-999999999|c\n", b"x.y:00|c\n"]
    n = 0
    for s in seeds:
        for at in range(len(s) + 1):
            for ch in alphabet:
                for line in (s[:at] + bytes([ch]) + s[at:], s[:at] + bytes([ch]) + s[at + 1:], s[:at] + s[at + 1:]):
                    assert pkg.coalesce_parse(line) == E.parse(line), line
                    n += 1
    for _ in range(3000):
        line = bytes(rng.choice(np.frombuffer(alphabet, np.uint8), int(rng.integers(0, 24))))
        assert pkg.coalesce_parse(line) == E.parse(line), line
    assert n > 4000


@pytest.mark.parametrize("total", [0, 1, -1, 9, 10, -10, 99, 100, 999999999, -999999999, 1000000000, 1 << 31, -(1 << 31),
                                   (1 << 60) - 1, -(1 << 60), (1 << 63) - 1, -(1 << 63), 10 ** 18, 10 ** 18 - 1])
def test_format_matches_the_restatement(pkg, total):
    for name in (b"a", b"svc.req.count", b"n\x00\xff", b"n" * 1425):
        line = pkg.coalesce_format(name, total)
        assert line == E.merged_line(name, total)
        assert E.MIN_LINE <= len(line) <= E.MAX_LINE
        if abs(total) <= 999999999:
            assert pkg.coalesce_parse(line) == (len(name), total)


def test_slot_limits(pkg):
    """The table size's limits are checked before the device is touched: a context is needed, so this only pins
    the constants the GPU tests use."""
    assert pkg.SR_COALESCE_MIN_SLOTS == 16 and pkg.SR_COALESCE_DEFAULT_SLOTS == 65536
    assert pkg.SR_COALESCE_MAX_SLOTS == 1 << 22 and pkg.SR_COALESCE_NAME_MAX + 24 == 1449
