"""The sample-rate stage's entry points: declared, listed, exported, the structures and constants the same in C and
Python, argument errors that need no device, and the host functions against tests/sample_expect.py: sr_sample_parse
over every single-byte mutation and every truncation of lines that together use every type and section, the ladder,
the keep rule, the rate texts, the rewrite, the specs and the configurations. CPU only: needs the built libraries,
calls no GPU code."""
from __future__ import annotations

import ctypes
import errno
import os
import random
import re
import subprocess

import pytest

import sample_expect as E
from conftest import REPO
from test_abi import _exported, declared_functions

NEW = {"sr_sample_open", "sr_sample_close", "sr_sample", "sr_sample_read", "sr_sample_reset", "sr_sample_check",
       "sr_sample_parse", "sr_sample_step", "sr_sample_keep", "sr_sample_rate_text", "sr_sample_rewrite", "sr_sample_parse_spec",
       "sr_set_sample", "sr_route_pack_sample"}


def test_new_functions_declared_listed_exported(pkg):
    assert NEW <= declared_functions()
    assert NEW <= set(pkg.ABI_FUNCTIONS)
    assert NEW <= _exported(pkg.ROUTE_LIB)
    lib = pkg.lib()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name
    for name in ("sample_open", "sample_close", "sample", "sample_batches", "sample_read", "sample_reset", "set_sample",
                 "route_pack_sample"):
        assert callable(getattr(pkg.Router, name)), name


def test_structures_and_constants_match_c(pkg, tmp_path):
    structs = {"sr_sample_config": pkg.SrSampleConfig, "sr_sample_batch": pkg.SrSampleBatch, "sr_sample_hits": pkg.SrSampleHits}
    consts = ["SR_SAMPLE_STEPS", "SR_SAMPLE_EXTRA_MAX", "SR_SAMPLE_LINE_MAX", "SR_SAMPLE_NOT_SAMPLEABLE", "SR_SAMPLE_DROPPED",
              "SR_SAMPLE_DEFAULT_SLOTS", "SR_SAMPLE_MIN_SLOTS", "SR_SAMPLE_MAX_SLOTS", "SR_SAMPLE_MAX_BYTES", "SR_SAMPLE_TYPES_ALL"]
    body, want = "", []
    for cname, py in structs.items():
        body += f'  printf(" %zu", sizeof({cname}));\n'
        want.append(ctypes.sizeof(py))
        for f, _ in py._fields_:
            body += f'  printf(" %zu", offsetof({cname}, {f}));\n'
            want.append(getattr(py, f).offset)
    for c in consts:
        body += f'  printf(" %lu", (unsigned long){c});\n'
        want.append(getattr(pkg, c))
    sizes = [0, 5, 6, 11, 12, 1 << 20, 1 << 30]
    for nb in sizes:
        body += f'  printf(" %zu", (size_t)SR_SAMPLE_APPEND_CAPACITY({nb}));\n'
        want.append(pkg.sample_append_capacity(nb))
    src = tmp_path / "sample.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sr_route.h"\nint main(void) {\n' + body
                   + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "sample"
    subprocess.run([os.environ.get("CC", "cc"), "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert out == want
    k = len(sizes)
    assert out[-k - 10:-k] == [E.STEPS, E.EXTRA_MAX, E.LINE_MAX, E.NOT_SAMPLEABLE, E.DROPPED, E.DEFAULT_SLOTS, 16, 1 << 22, 1 << 30,
                               E.TYPES_ALL]
    assert out[-k:] == [E.append_capacity(nb) for nb in sizes]
    assert ctypes.sizeof(pkg.SrSampleConfig) == 24 and ctypes.sizeof(pkg.SrSampleBatch) == 96


def test_tile_constant_is_the_kernels(pkg):
    src = open(os.path.join(REPO, "statsd-router_amd", "csrc", "sample_kernel.hpp")).read()
    block = int(re.search(r"constexpr int kSampleBlock = (\d+);", src).group(1))
    assert re.search(r"constexpr int kSampleTile = kSampleBlock;", src)
    assert pkg.SAMPLE_TILE == block


def test_argument_errors_need_no_device(pkg):
    lib = pkg.lib()
    cfg = pkg.SampleConfig(4)
    b = (pkg.SrSampleBatch * 1)()
    h = (pkg.SrSampleHits * 2)()
    u = ctypes.c_uint32()
    assert lib.sr_sample_open(None, cfg.ref()) == -errno.EINVAL
    assert lib.sr_sample_close(None) == -errno.EINVAL
    assert lib.sr_sample(None, b, 1) == -errno.EINVAL
    assert lib.sr_sample_read(None, h, 2) == -errno.EINVAL
    assert lib.sr_sample_reset(None) == -errno.EINVAL
    assert lib.sr_sample_check(None) == -errno.EINVAL
    assert lib.sr_set_sample(None, cfg.ref()) == -errno.EINVAL
    text, n, c4, seed = ctypes.c_void_p(), ctypes.c_size_t(), (ctypes.c_uint64 * 4)(), ctypes.c_uint64()
    assert lib.sr_route_pack_sample(None, 0, ctypes.byref(text), ctypes.byref(n), c4, ctypes.byref(seed)) == -errno.EINVAL
    assert lib.sr_sample_parse(None, 6, 1, ctypes.byref(u), ctypes.byref(u)) == -errno.EINVAL
    assert lib.sr_sample_parse(b"a:1|c\n", 6, 1, None, None) == 1 and lib.sr_sample_parse(b"a:1|c\n", 0, 1, None, None) == 0
    assert lib.sr_sample_keep(1, 2, 3, 13) == -errno.EINVAL and lib.sr_sample_keep(1, 2, 3, 0) == 1
    assert lib.sr_sample_parse_spec(None, cfg.ref()) == -errno.EINVAL
    assert lib.sr_sample_parse_spec(b"4", None) == -errno.EINVAL
    assert lib.sr_sample_rewrite(None, b"a:1|c\n", 6, 5, 1) == 0


def test_configurations(pkg):
    good = [(0, 1, 4, 0), (16, 1, 1, 0), (1 << 22, 0xFFFFFFFF, E.TYPES_ALL, 0), (65536, 7, 32 | 8, 0)]
    bad = [(8, 1, 4, 0), (15, 1, 4, 0), (48, 1, 4, 0), (1 << 23, 1, 4, 0), (0, 0, 4, 0), (0, 1, 0, 0), (0, 1, 2, 0), (0, 1, 16, 0),
           (0, 1, 64, 0), (0, 1, 1 << 31, 0), (0, 1, 4, 1)]
    for slots, limit, types, reserved in good:
        assert E.check(slots, limit, types, reserved)
        assert pkg.SampleConfig(limit, types, slots, 5, reserved).check() == 0
    for slots, limit, types, reserved in bad:
        assert not E.check(slots, limit, types, reserved)
        assert pkg.SampleConfig(limit, types, slots, 5, reserved).check() == -errno.EINVAL


def test_parse_against_the_restatement_over_every_mutation_and_truncation(pkg):
    """256 values at each position of each line and each line cut after every byte, each also behind 0..32 bytes of
    a longer name, so that ':' and both '|' meet every edge of a 16-byte step: the C function, which walks steps with
    masks, and the restatement, which uses bytes.find, agree on every one, under every type and under `ms` alone."""
    lib = pkg.lib()
    ins, bit = ctypes.c_uint32(), ctypes.c_uint32()
    n = sampleable = 0
    for ln in E.SEED_LINES:
        cands = [ln[:k] for k in range(1, len(ln) + 1)]
        cands += [ln[:at] + bytes([v]) + ln[at + 1:] for at in range(len(ln)) for v in range(256) if v != ln[at]]
        for pad in range(33):
            cands += [b"n" * pad + ln, b"n" * pad + ln[:-1] + b"|#t\n", b"n" * pad + ln[:-1] + b"|\n"]
        for c in cands:
            for types in (E.TYPES_ALL, 4):
                rc = lib.sr_sample_parse(c, len(c), types, ctypes.byref(ins), ctypes.byref(bit))
                want = E.parse(c, types)
                assert (None if rc == 0 else (ins.value, bit.value)) == want and rc in (0, 1), (c, types)
                n += 1
                sampleable += want is not None
    assert n > 90000 and sampleable > 10000


def test_long_lines(pkg):
    for ln in (b"a:" + b"1" * 1436 + b"|h\n", b"a:" + b"1" * 1437 + b"|h\n", b"n" * 1435 + b":1|c\n", b"n" * 1436 + b":1|c\n",
               b"a:1|ms|#" + b"t" * 1432 + b"\n", b"a:1|" + b"m" * 1400 + b"\n", b"a:1|ms" + b"|" * 1000 + b"\n",
               b"n" * 1000 + b"|" + b"n" * 400 + b":1|d\n", b"a:" + b"|" * 1400 + b"\n"):
        assert pkg.sample_parse(ln) == E.parse(ln), ln[:20]


def test_the_ladder(pkg):
    for limit in (1, 3, 1000, 0xFFFFFFFF):
        for j, k in enumerate(E.K):
            for c in (limit * k - 1, limit * k, limit * k + 1):
                assert pkg.sample_step(limit, c) == E.step(limit, c), (limit, c)
        assert pkg.sample_step(limit, 0) == 0 and pkg.sample_step(limit, (1 << 64) - 1) == E.step(limit, (1 << 64) - 1)


def test_the_keep_rule(pkg):
    rnd = random.Random(5)
    for _ in range(20000):
        h, seed, i, j = rnd.getrandbits(64), rnd.getrandbits(64), rnd.getrandbits(rnd.choice((8, 20, 33, 64))), rnd.randrange(13)
        assert pkg.sample_keep(h, seed, i, j) == E.keep(h, seed, i, j), (h, seed, i, j)


def test_rate_texts_and_rewrites(pkg):
    assert [pkg.sample_rate_text(j).encode() for j in range(E.STEPS)] == E.R
    assert pkg.sample_rate_text(E.STEPS) is None and pkg.sample_rate_text(0xFF) is None
    for ln in (b"a:1|c\n", b"abc:12|ms|#t\n", b"a:" + b"1" * 1436 + b"|h\n"):
        ins = E.parse(ln)[0]
        for j in range(1, E.STEPS):
            assert pkg.sample_rewrite(ln, ins, j) == E.rewrite(ln, ins, j)
        assert pkg.sample_rewrite(ln, ins, 0) == b"" and pkg.sample_rewrite(ln, ins, 13) == b""
        assert pkg.sample_rewrite(ln, len(ln) + 1, 1) == b""
    assert len(pkg.sample_rewrite(b"a:" + b"1" * 1436 + b"|h\n", 1440, 12)) == 1449


def test_parse_spec(pkg):
    for spec in ("4", "1", "4294967295", "1000:c", "7:ms,h,d,c", "5:d,d", "12:ms", "3:h,c"):
        cfg = pkg.sample_parse_spec(spec)
        assert (cfg.limit, cfg.types) == E.parse_spec(spec), spec
        assert cfg.slots == 0 and cfg.seed == 0 and cfg.check() == 0
    for bad in ("", "0", "-1", "+4", "4:", "4:x", "4:c,", "4:,c", "4:C", "4 ", " 4", "4:c ms", "4294967296", "4:g", "4:s", "x", "4;c",
                "99999999999999999999999"):
        assert E.parse_spec(bad) is None, bad
        with pytest.raises(pkg.SrError) as ei:
            pkg.sample_parse_spec(bad)
        assert ei.value.errno == errno.EINVAL, bad
