"""The rules kernels (statsd-router_amd/csrc/rules_kernel.hpp) in the built library's code-object metadata (no GPU
needed): each is there, uses no scratch and spills no register, and has the workgroup size, the fixed LDS and the
register ceiling that DESIGN.md §5.11 states."""
from __future__ import annotations

import pytest

import code_object as C

TILES = 272    # every tiled kernel: the batches' record counts and first tiles (u32 [32], u32 [33]) as laid out
TABLE = 9760   # sizeof(RulesTable): header, 256 keys, 256 entries, actions, first bytes, 4096 text bytes
# symbol -> (workgroup size, fixed LDS bytes)
RULES_KERNELS = {
    # the table, 257 x {lines, bytes} u64 hit cells, four waves' {kept, dropped, bytes, subject}
    "_ZN3srk18rules_match_kernelENS_9RulesArgsE": (256, TABLE + 257 * 2 * 8 + TILES + 4 * 4 * 4),
    # sixteen waves' {kept, dropped, subject} and their dropped bytes (u64)
    "_ZN3srk17rules_scan_kernelENS_9RulesArgsE": (1024, TILES + 16 * 3 * 4 + 16 * 8),
    # the actions, four waves' kept counts
    "_ZN3srk17rules_emit_kernelENS_9RulesArgsE": (256, 272 + TILES + 4 * 4),
    # the host-memory path's copy into page-locked memory: no LDS
    "_ZN3srk16rules_out_kernelENS_8RulesOutE": (256, 0),
}


@pytest.fixture(scope="module")
def kernel_meta(tmp_path_factory):
    co = C.extract(tmp_path_factory.mktemp("co"))
    assert co, "llvm-objcopy / clang-offload-bundler not found"
    meta = C.metadata(co)
    assert meta, "no kernel metadata in the code object (llvm-readelf?)"
    return meta


@pytest.mark.parametrize("sym", sorted(RULES_KERNELS))
def test_rules_kernels_use_no_scratch(kernel_meta, sym):
    assert sym in kernel_meta, f"{sym} is not in the library"
    m = kernel_meta[sym]
    print({k: m[k] for k in ("sgpr_count", "vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                             "sgpr_spill_count", "vgpr_spill_count")})
    assert m["private_segment_fixed_size"] == 0
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
    size, lds = RULES_KERNELS[sym]
    assert m["max_flat_workgroup_size"] == size
    assert m["group_segment_fixed_size"] == lds


# the vector registers DESIGN.md §5.11 quotes: the build may use fewer, never more
VGPRS = {"_ZN3srk18rules_match_kernelENS_9RulesArgsE": 48, "_ZN3srk17rules_scan_kernelENS_9RulesArgsE": 117,
         "_ZN3srk17rules_emit_kernelENS_9RulesArgsE": 20, "_ZN3srk16rules_out_kernelENS_8RulesOutE": 10}


@pytest.mark.parametrize("sym", sorted(VGPRS))
def test_registers_are_those_quoted(kernel_meta, sym):
    assert kernel_meta[sym]["vgpr_count"] <= VGPRS[sym]


def test_eight_workgroups_fit_a_cu(kernel_meta):
    """256 threads and at most 64 registers: eight workgroups of every tiled kernel are resident on a CU (two
    waves of each per SIMD), LDS included, which is what the grid's limit of 2048 workgroups assumes."""
    for sym, (size, lds) in RULES_KERNELS.items():
        if size == 256:
            assert kernel_meta[sym]["vgpr_count"] <= 64 and 8 * lds <= 160 * 1024


def test_the_scan_kernel_fits_its_one_workgroup(kernel_meta):
    """1024 threads are four waves per SIMD: at most 128 registers each."""
    assert kernel_meta["_ZN3srk17rules_scan_kernelENS_9RulesArgsE"]["vgpr_count"] <= 128


def test_there_are_no_other_rules_kernels(kernel_meta):
    assert {k for k in kernel_meta if "rules_" in k} == set(RULES_KERNELS)
