"""The coalescing kernels (statsd-router_amd/csrc/coalesce_kernel.hpp) in the built library's code-object
metadata (no GPU needed): each is there, uses no scratch and spills no register, and has the workgroup size and
the fixed LDS that DESIGN.md §5.10 states."""
from __future__ import annotations

import pytest

import code_object as C

# symbol -> (workgroup size, fixed LDS bytes)
TILES = 272   # every tiled kernel: the batches' record counts and first tiles (u32 [32], u32 [33]) as the compiler lays them out
COALESCE_KERNELS = {
    "_ZN3srk21coalesce_clear_kernelEPNS_12CoalesceSlotEj": (256, 0),
    "_ZN3srk21coalesce_claim_kernelENS_12CoalesceArgsE": (256, TILES),
    "_ZN3srk20coalesce_join_kernelENS_12CoalesceArgsE": (256, TILES),
    # four waves' {kept, groups, bytes}
    "_ZN3srk19coalesce_sum_kernelENS_12CoalesceArgsE": (256, TILES + 4 * 3 * 4),
    # sixteen waves' {kept, groups, bytes}
    "_ZN3srk20coalesce_scan_kernelENS_12CoalesceArgsE": (1024, TILES + 16 * 3 * 4),
    # four waves' {kept, bytes}
    "_ZN3srk20coalesce_emit_kernelENS_12CoalesceArgsE": (256, TILES + 4 * 2 * 4),
    # the host-memory path's copy into page-locked memory: no LDS
    "_ZN3srk19coalesce_out_kernelENS_11CoalesceOutE": (256, 0),
}


@pytest.fixture(scope="module")
def kernel_meta(tmp_path_factory):
    co = C.extract(tmp_path_factory.mktemp("co"))
    assert co, "llvm-objcopy / clang-offload-bundler not found"
    meta = C.metadata(co)
    assert meta, "no kernel metadata in the code object (llvm-readelf?)"
    return meta


@pytest.mark.parametrize("sym", sorted(COALESCE_KERNELS))
def test_coalesce_kernels_use_no_scratch(kernel_meta, sym):
    assert sym in kernel_meta, f"{sym} is not in the library"
    m = kernel_meta[sym]
    print({k: m[k] for k in ("sgpr_count", "vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                             "sgpr_spill_count", "vgpr_spill_count")})
    assert m["private_segment_fixed_size"] == 0
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
    size, lds = COALESCE_KERNELS[sym]
    assert m["max_flat_workgroup_size"] == size
    assert m["group_segment_fixed_size"] == lds


def test_eight_workgroups_fit_a_cu(kernel_meta):
    """256 threads and at most 64 registers: eight workgroups of every tiled kernel are resident on a CU (two
    waves of each per SIMD), which is what the grid's limit of 2048 workgroups assumes."""
    for sym, (size, lds) in COALESCE_KERNELS.items():
        if size == 256:
            assert kernel_meta[sym]["vgpr_count"] <= 64 and 8 * lds <= 160 * 1024


def test_there_are_no_other_coalesce_kernels(kernel_meta):
    assert {k for k in kernel_meta if "coalesce_" in k} == set(COALESCE_KERNELS)
