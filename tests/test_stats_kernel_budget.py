"""The name-statistics kernels (statsd-router_amd/csrc/stats_kernel.hpp) in the built library's code-object
metadata (no GPU needed): each is there, uses no scratch and spills no register, and has the workgroup size and
the fixed LDS that DESIGN.md §5.9 states (the counting kernel's sketch is dynamic LDS on top: 4 bytes per cell,
at most 64 KiB)."""
from __future__ import annotations

import pytest

import code_object as C

# symbol -> (workgroup size, fixed LDS bytes)
TILES = 272   # every kernel: the batches' record counts and first tiles (u32 [32], u32 [33]) as the compiler lays them out
STATS_KERNELS = {
    # per-shard sums in LDS: 2 x 512 u64 + 9 u64 of per-verdict sums
    "_ZN3srk18stats_count_kernelILb1EEEvNS_9StatsArgsE": (1024, 2 * 512 * 8 + 9 * 8 + TILES),
    # more than 512 shards: the per-verdict sums alone
    "_ZN3srk18stats_count_kernelILb0EEEvNS_9StatsArgsE": (1024, 9 * 8 + TILES),
    # one bit per cell (16384 / 8), 256 remembered names (u64) and their flags (u32)
    "_ZN3srk16stats_hot_kernelENS_9StatsArgsE": (1024, 2048 + 256 * 8 + 256 * 4 + TILES),
}


@pytest.fixture(scope="module")
def kernel_meta(tmp_path_factory):
    co = C.extract(tmp_path_factory.mktemp("co"))
    assert co, "llvm-objcopy / clang-offload-bundler not found"
    meta = C.metadata(co)
    assert meta, "no kernel metadata in the code object (llvm-readelf?)"
    return meta


@pytest.mark.parametrize("sym", sorted(STATS_KERNELS))
def test_stats_kernels_use_no_scratch(kernel_meta, sym):
    assert sym in kernel_meta, f"{sym} is not in the library"
    m = kernel_meta[sym]
    print({k: m[k] for k in ("sgpr_count", "vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                             "sgpr_spill_count", "vgpr_spill_count")})
    assert m["private_segment_fixed_size"] == 0
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
    size, lds = STATS_KERNELS[sym]
    assert m["max_flat_workgroup_size"] == size
    assert m["group_segment_fixed_size"] == lds


def test_two_counting_workgroups_fit_a_cu(kernel_meta, pkg):
    """The largest sketch (64 KiB of u32 cells) next to the fixed LDS leaves room for two workgroups in a CU's
    160 KiB, and the registers for the four waves per SIMD of one 1024-thread workgroup."""
    m = kernel_meta["_ZN3srk18stats_count_kernelILb1EEEvNS_9StatsArgsE"]
    assert 2 * (m["group_segment_fixed_size"] + 4 * pkg.SR_STATS_MAX_CELLS) <= 160 * 1024
    assert m["vgpr_count"] <= 128
    assert kernel_meta["_ZN3srk16stats_hot_kernelENS_9StatsArgsE"]["vgpr_count"] <= 128


def test_there_are_no_other_stats_kernels(kernel_meta):
    assert {k for k in kernel_meta if "stats_" in k} == set(STATS_KERNELS)
