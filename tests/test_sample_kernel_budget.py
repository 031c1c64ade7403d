"""The sample-rate kernels (statsd-router_amd/csrc/sample_kernel.hpp) in the built library's code-object metadata (no
GPU needed): each is there, uses no scratch and spills no register, and has the workgroup size, the fixed LDS and
the register ceiling that DESIGN.md §5.13 states."""
from __future__ import annotations

import pytest

import code_object as C

TILES = 272    # every tiled kernel: the batches' record counts and first tiles (u32 [32], u32 [33]) as laid out
# symbol -> (workgroup size, fixed LDS bytes)
SAMPLE_KERNELS = {
    # the table's words to zero: no LDS
    "_ZN3srk19sample_clear_kernelENS_10SampleArgsE": (256, 0),
    # the parse and the slot counts: the tile numbering only
    "_ZN3srk19sample_count_kernelENS_10SampleArgsE": (256, TILES),
    # 13 x {seen, kept} u64 hit cells, four waves' {kept, rewritten, bytes, dropped}
    "_ZN3srk17sample_sum_kernelENS_10SampleArgsE": (256, 13 * 2 * 8 + TILES + 4 * 4 * 4),
    # sixteen waves' {kept, rewritten, bytes, dropped}
    "_ZN3srk18sample_scan_kernelENS_10SampleArgsE": (1024, TILES + 16 * 4 * 4),
    # four waves' {kept, rewritten bytes}
    "_ZN3srk18sample_emit_kernelENS_10SampleArgsE": (256, TILES + 4 * 2 * 4),
    # the host-memory path's copy into page-locked memory: no LDS
    "_ZN3srk17sample_out_kernelENS_9SampleOutE": (256, 0),
}


@pytest.fixture(scope="module")
def kernel_meta(tmp_path_factory):
    co = C.extract(tmp_path_factory.mktemp("co"))
    assert co, "llvm-objcopy / clang-offload-bundler not found"
    meta = C.metadata(co)
    assert meta, "no kernel metadata in the code object (llvm-readelf?)"
    return meta


@pytest.mark.parametrize("sym", sorted(SAMPLE_KERNELS))
def test_sample_kernels_use_no_scratch(kernel_meta, sym):
    assert sym in kernel_meta, f"{sym} is not in the library"
    m = kernel_meta[sym]
    print({k: m[k] for k in ("sgpr_count", "vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                             "sgpr_spill_count", "vgpr_spill_count")})
    assert m["private_segment_fixed_size"] == 0
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
    size, lds = SAMPLE_KERNELS[sym]
    assert m["max_flat_workgroup_size"] == size
    assert m["group_segment_fixed_size"] == lds


# the vector registers DESIGN.md §5.13 quotes: the build may use fewer, never more
VGPRS = {"_ZN3srk19sample_clear_kernelENS_10SampleArgsE": 8, "_ZN3srk19sample_count_kernelENS_10SampleArgsE": 52,
         "_ZN3srk17sample_sum_kernelENS_10SampleArgsE": 34, "_ZN3srk18sample_scan_kernelENS_10SampleArgsE": 93,
         "_ZN3srk18sample_emit_kernelENS_10SampleArgsE": 44, "_ZN3srk17sample_out_kernelENS_9SampleOutE": 14}


@pytest.mark.parametrize("sym", sorted(VGPRS))
def test_registers_are_those_quoted(kernel_meta, sym):
    assert kernel_meta[sym]["vgpr_count"] <= VGPRS[sym]


def test_eight_workgroups_fit_a_cu(kernel_meta):
    """256 threads, at most 64 vector and 96 scalar registers: eight workgroups of every tiled kernel are resident
    on a CU (eight waves per SIMD, one of each workgroup; 8 x 96 of a SIMD's 800 scalar registers), LDS included,
    which is what the grid's limit of 2048 workgroups assumes."""
    for sym, (size, lds) in SAMPLE_KERNELS.items():
        if size == 256:
            m = kernel_meta[sym]
            assert m["vgpr_count"] <= 64 and m["sgpr_count"] <= 96 and 8 * lds <= 160 * 1024


def test_the_scan_kernel_fits_its_one_workgroup(kernel_meta):
    """1024 threads are four waves per SIMD: at most 128 registers each."""
    assert kernel_meta["_ZN3srk18sample_scan_kernelENS_10SampleArgsE"]["vgpr_count"] <= 128


def test_there_are_no_other_sample_kernels(kernel_meta):
    assert {k for k in kernel_meta if "sample_" in k} == set(SAMPLE_KERNELS)
