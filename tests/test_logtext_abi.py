"""The device-log entry point (sr_format_log): declared, listed, exported, the structure and the capacity
macros the same in C and Python. CPU only: needs the built library, calls no GPU code."""
from __future__ import annotations

import ctypes
import errno
import importlib
import os
import subprocess

import log_expect as L
from conftest import REPO
from test_abi import _exported, declared_functions

NEW_ROUTE = {"sr_format_log", "sr_set_logtext", "sr_route_pack_set_prefix", "sr_route_pack_set_ends",
             "sr_route_pack_logtext"}
NEW_CORE = {"sr_core_set_device_log", "sr_core_device_log_stats"}
FIELDS = ("d_bytes", "nbytes", "d_recs", "d_n_records", "max_records", "d_hashes", "d_ends", "n_datagrams",
          "min_level", "d_prefix", "prefix_len", "max_msg", "d_text", "text_cap", "d_offsets", "d_levels", "max_msgs",
          "d_total", "d_n_msgs")


def test_new_functions_declared_listed_exported(pkg):
    assert NEW_ROUTE <= declared_functions()
    assert NEW_ROUTE <= set(pkg.ABI_FUNCTIONS)
    assert NEW_ROUTE <= _exported(pkg.ROUTE_LIB)
    lib = pkg.lib()
    for name in NEW_ROUTE:
        assert getattr(lib, name).argtypes is not None, name
    for name in ("format_log", "set_logtext", "route_pack_set_prefix", "route_pack_set_ends", "route_pack_logtext"):
        assert callable(getattr(pkg.Router, name)), name
    core = importlib.import_module("statsd-router_amd.core")
    core.router_lib()
    assert NEW_CORE <= declared_functions("sr_router.h")
    assert NEW_CORE <= _exported(core.ROUTER_LIB)
    assert callable(core.Core.set_device_log) and callable(core.Core.device_log_stats)


def test_structure_and_macros_match_c(pkg, tmp_path):
    src = tmp_path / "sizes.c"
    offs = ", ".join(f"offsetof(sr_log_batch, {f})" for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include "sr_route.h"\n'
                   'int main(void) { size_t o[] = {%s}; printf("%%zu %%u %%llu %%llu %%llu", sizeof(sr_log_batch), '
                   'SR_LOG_MAX_PREFIX, (unsigned long long)SR_LOG_MAX_MSGS(1000003, 77), '
                   '(unsigned long long)SR_LOG_TEXT_CAPACITY(1000003, 77, 35), '
                   '(unsigned long long)SR_LOG_TEXT_CAPACITY(0xFFFFFFF0u, 0xFFFFFFF0u, 256u)); '
                   'for (unsigned i = 0; i < sizeof o / sizeof *o; i++) printf(" %%zu", o[i]); return 0; }\n' % offs)
    exe = tmp_path / "sizes"
    subprocess.run([os.environ.get("CC", "cc"), "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    size, pmax, msgs, cap, big = out[:5]
    assert ctypes.sizeof(pkg.SrLogBatch) == size
    assert [getattr(pkg.SrLogBatch, f).offset for f in FIELDS] == out[5:]
    assert pkg.SR_LOG_MAX_PREFIX == pmax == 256
    assert pkg.log_max_msgs(1000003, 77) == msgs == L.max_msgs(1000003, 77) == 1000080
    assert pkg.log_text_capacity(1000003, 77, 35) == cap == L.text_capacity(1000003, 77, 35) == 1000003 * 78 + 77 * 60
    assert big == pkg.log_text_capacity(0xFFFFFFF0, 0xFFFFFFF0, 256)   # the macros compute in 64 bits


def test_null_arguments_are_refused_without_a_device(pkg):
    assert pkg.lib().sr_format_log(None, None) == -errno.EINVAL
    assert pkg.lib().sr_format_log(None, ctypes.byref(pkg.SrLogBatch())) == -errno.EINVAL
