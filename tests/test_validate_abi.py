"""The line grammar's entry points: declared, listed, exported, the structures and constants the same in C and
Python, argument errors that need no device, sr_validate_line against tests/validate_expect.py (every single-byte
mutation and every truncation of ten lines that together use every section), the reasons' names, the specs that
sr_validate_parse_spec takes and refuses, and the configurations that are -EINVAL. CPU only: needs the built
libraries, calls no GPU code."""
from __future__ import annotations

import ctypes
import errno
import os
import re
import subprocess

import pytest

import validate_expect as E
from conftest import REPO
from test_abi import _exported, declared_functions

NEW = {"sr_validate_open", "sr_validate_close", "sr_validate", "sr_validate_read", "sr_validate_reset", "sr_validate_check",
       "sr_validate_line", "sr_validate_reason_name", "sr_validate_parse_spec", "sr_set_validate", "sr_route_pack_validate"}


def test_new_functions_declared_listed_exported(pkg):
    assert NEW <= declared_functions()
    assert NEW <= set(pkg.ABI_FUNCTIONS)
    assert NEW <= _exported(pkg.ROUTE_LIB)
    lib = pkg.lib()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name
    for name in ("validate_open", "validate_close", "validate", "validate_batches", "validate_read", "validate_reset",
                 "set_validate", "route_pack_validate"):
        assert callable(getattr(pkg.Router, name)), name


def test_structures_and_constants_match_c(pkg, tmp_path):
    structs = {"sr_validate_config": pkg.SrValidateConfig, "sr_validate_batch": pkg.SrValidateBatch,
               "sr_validate_hits": pkg.SrValidateHits}
    consts = ["SR_VALID_OK", "SR_VALID_NO_COLON", "SR_VALID_EMPTY_NAME", "SR_VALID_NAME_BYTE", "SR_VALID_NO_TYPE",
              "SR_VALID_TYPE", "SR_VALID_VALUE", "SR_VALID_SECTION", "SR_VALID_RATE", "SR_VALID_TAGS", "SR_VALID_REASONS",
              "SR_VALID_NOT_SUBJECT", "SR_VALID_TYPE_C", "SR_VALID_TYPE_G", "SR_VALID_TYPE_MS", "SR_VALID_TYPE_H",
              "SR_VALID_TYPE_S", "SR_VALID_TYPE_D", "SR_VALID_TYPES_ALL"]
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
    src = tmp_path / "validate.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sr_route.h"\nint main(void) {\n' + body
                   + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "validate"
    subprocess.run([os.environ.get("CC", "cc"), "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert out == want
    assert tuple(out[-19:-7]) == (E.OK, E.NO_COLON, E.EMPTY_NAME, E.NAME_BYTE, E.NO_TYPE, E.TYPE, E.VALUE, E.SECTION,
                                  E.RATE, E.TAGS, E.REASONS, E.NOT_SUBJECT)
    assert out[-7:-1] == [E.TYPE_BITS[t] for t in (b"c", b"g", b"ms", b"h", b"s", b"d")] and out[-1] == E.TYPES_ALL
    assert pkg.SR_VALID_DROP_ALL == E.DROP_ALL


def test_tile_constant_is_the_kernels(pkg):
    src = open(os.path.join(REPO, "statsd-router_amd", "csrc", "validate_kernel.hpp")).read()
    block = int(re.search(r"constexpr int kValidBlock = (\d+);", src).group(1))
    assert re.search(r"constexpr int kValidTile = kValidBlock;", src)
    assert pkg.VALIDATE_TILE == block


def test_argument_errors_need_no_device(pkg):
    lib = pkg.lib()
    cfg = pkg.ValidateConfig()
    b = (pkg.SrValidateBatch * 1)()
    h = (pkg.SrValidateHits * 2)()
    c4 = (ctypes.c_uint64 * 4)()
    assert lib.sr_validate_open(None, cfg.ref()) == -errno.EINVAL
    assert lib.sr_validate_close(None) == -errno.EINVAL
    assert lib.sr_validate(None, b, 1) == -errno.EINVAL
    assert lib.sr_validate_read(None, h, 2) == -errno.EINVAL
    assert lib.sr_validate_reset(None) == -errno.EINVAL
    assert lib.sr_set_validate(None, cfg.ref()) == -errno.EINVAL
    assert lib.sr_route_pack_validate(None, 0, c4) == -errno.EINVAL
    assert lib.sr_validate_line(None, b"a:1|c\n", 6) == -errno.EINVAL
    assert lib.sr_validate_line(cfg.ref(), None, 6) == -errno.EINVAL
    assert lib.sr_validate_line(cfg.ref(), b"a:1|c\n", 0) == -errno.EINVAL
    assert lib.sr_validate_line(cfg.ref(), b"a:1|c\n", 6) == 0
    assert lib.sr_validate_parse_spec(None, cfg.ref()) == -errno.EINVAL
    assert lib.sr_validate_parse_spec(b"drop", None) == -errno.EINVAL
    assert lib.sr_validate_check(None) == -errno.EINVAL


def test_configurations(pkg):
    for mask, types in ((0, 63), (0x3FE, 63), (1 << 9, 32), (2, 1), (0, 1), (0x3FE, 21)):
        assert E.check(mask, types) and pkg.ValidateConfig(mask, types).check() == 0, (mask, types)
    for mask, types in ((1, 63), (3, 63), (1 << 10, 63), (1 << 31, 63), (0x7FE, 63), (0, 0), (0x3FE, 0), (0, 64), (0, 0xFF),
                        (0, 1 << 31)):
        assert not E.check(mask, types) and pkg.ValidateConfig(mask, types).check() == -errno.EINVAL, (mask, types)
        with pytest.raises(pkg.SrError):
            pkg.ValidateConfig(mask, types).line(b"a:1|c\n")


def test_reason_names(pkg):
    assert [pkg.validate_reason_name(r) for r in range(E.REASONS)] == E.NAMES
    assert pkg.validate_reason_name(E.REASONS) is None and pkg.validate_reason_name(E.NOT_SUBJECT) is None


def test_parse_spec_round_trips(pkg):
    specs = ["count", "drop"] + E.NAMES[1:] + ["value,tags", ",".join(E.NAMES[1:]), "tags,no_colon,tags", "rate,type"]
    for spec in specs:
        cfg = pkg.validate_parse_spec(spec)
        assert (cfg.drop_mask, cfg.accept_types) == E.parse_spec(spec), spec
        assert cfg.check() == 0
        # the mask back into names and through the parser again
        names = ",".join(E.NAMES[r] for r in range(1, E.REASONS) if cfg.drop_mask >> r & 1)
        if names:
            assert pkg.validate_parse_spec(names).drop_mask == cfg.drop_mask
    assert pkg.validate_parse_spec("drop").drop_mask == pkg.validate_parse_spec(",".join(E.NAMES[1:])).drop_mask
    for bad in ("", "ok", "value,", ",value", "value,,tags", "Value", "DROP", "drop,count", "count,value", "value tags", " drop",
                "drop ", "valu", "values", "0x3fe", "all"):
        assert E.parse_spec(bad) is None, bad
        with pytest.raises(pkg.SrError) as ei:
            pkg.validate_parse_spec(bad)
        assert ei.value.errno == errno.EINVAL, bad


def test_seed_lines_use_every_section_and_are_ok(pkg):
    cfg = pkg.ValidateConfig()
    text = b"".join(E.SEED_LINES)
    assert all(cfg.line(ln) == E.OK == E.judge(ln) for ln in E.SEED_LINES)
    for piece in (b"|c", b"|g", b"|ms", b"|h", b"|s", b"|d", b"|@", b"|#", b"-", b"+", b"."):
        assert piece in text, piece
    assert any(not ln.endswith(b"\n") for ln in E.SEED_LINES)


def test_line_against_the_restatement_over_every_mutation_and_truncation(pkg):
    """256 values at each position of each line, and each line cut after every byte: the C function, which walks
    16-byte steps with masks, and the restatement, which splits and matches, give the same reason for all of them."""
    lib = pkg.lib()
    cfg = pkg.ValidateConfig()
    ref = cfg.ref()
    n = 0
    seen = set()
    for ln in E.mutations():
        got, want = lib.sr_validate_line(ref, ln, len(ln)), E.judge(ln)
        assert got == want, (ln, got, want)
        seen.add(want)
        n += 1
    assert n > 60000 and seen == set(range(E.REASONS))


@pytest.mark.parametrize("types", [1, 2 | 4, 63 & ~16, 32])
def test_line_with_an_accept_types_subset(pkg, types):
    lib = pkg.lib()
    ref = pkg.ValidateConfig(0, types).ref()
    for ln in E.SEED_LINES + [b"a:x|q", b"a:x|ms", b"a:1|c|@1", b"a:1|d|@x"]:
        assert lib.sr_validate_line(ref, ln, len(ln)) == E.judge(ln, types), ln


def test_long_lines(pkg):
    cfg = pkg.ValidateConfig()
    for ln in (b"n" * 1448 + b"\n", b"n" * 1449, b"n" * 1443 + b":1|c\n", b"a:1|c|#" + b"t" * 1441 + b"\n",
               b"a:1|c|#" + b"t" * 1000 + b" " + b"t" * 440 + b"\n", b"a:1|c|#" + b"t" * 1440 + b"|\n",
               b"n" * 700 + b" " + b"n" * 700 + b":1|c\n", b"a:" + b"1" * 1400 + b"|c\n", b"a:1|" + b"c" * 1400 + b"\n",
               b"a:1|c|@" + b"1" * 1400 + b"\n"):
        assert cfg.line(ln) == E.judge(ln), ln[:20]
