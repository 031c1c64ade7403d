"""The three log kernels (statsd-router_amd/csrc/log_kernel.hpp) in the built library's code-object metadata
(no GPU needed): each is there, uses no scratch and spills no register, and the writer stays within what lets
four of its workgroups share a CU's LDS."""
from __future__ import annotations

import pytest

import code_object as C

LOG_KERNELS = {
    "_ZN3srk15log_lens_kernelENS_7LogArgsE": 128,
    "_ZN3srk15log_scan_kernelENS_7LogArgsE": 1024,
    "_ZN3srk16log_write_kernelENS_7LogArgsE": 128,
}


@pytest.fixture(scope="module")
def kernel_meta(tmp_path_factory):
    co = C.extract(tmp_path_factory.mktemp("co"))
    assert co, "llvm-objcopy / clang-offload-bundler not found"
    meta = C.metadata(co)
    assert meta, "no kernel metadata in the code object (llvm-readelf?)"
    return meta


@pytest.mark.parametrize("sym", sorted(LOG_KERNELS))
def test_log_kernels_use_no_scratch(kernel_meta, sym):
    assert sym in kernel_meta, f"{sym} is not in the library"
    m = kernel_meta[sym]
    print({k: m[k] for k in ("sgpr_count", "vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                             "sgpr_spill_count", "vgpr_spill_count")})
    assert m["private_segment_fixed_size"] == 0
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
    assert m["max_flat_workgroup_size"] == LOG_KERNELS[sym]


def test_writer_budget(kernel_meta):
    m = kernel_meta["_ZN3srk16log_write_kernelENS_7LogArgsE"]
    assert m["vgpr_count"] <= 64 and m["group_segment_fixed_size"] <= 40960
