"""The budgets of the chunk-layout route kernels and of the uniform KV_DEFER1 variant, and which of them
hash on the matrix cores, read from the built library's gfx950 code object (no GPU needed).

Seven 256-thread workgroups per CU: at most 72 VGPRs, 96 SGPRs and 23,040 bytes of LDS, no scratch and
no VGPR spill. route_chunk_kernel<KV_CHUNKS | KV_ALIVE> and <KV_CHUNKS | KV_DEFER1> compute U(l), the
hash of the 64 bytes a lane loaded, with eight v_mfma_i32_16x16x64_i8 (sdbm_mx_row); the general and
KV_DEAD1 variants, whose pad dwords hold the probe's tables and marks, keep the VALU Horner."""
from __future__ import annotations

import os

import pytest

import code_object as CO

CHUNK = "_ZN3srk18route_chunk_kernelILj%dEEEvNS_11RouteParamsE"
KV_CHUNKS, KV_ALIVE, KV_DEFER1, KV_DEAD1, KV_PICKS = 1 << 23, 1 << 28, 1 << 31, 1 << 27, 1 << 29
CHUNK_MATRIX = [CHUNK % (KV_CHUNKS | KV_ALIVE), CHUNK % (KV_CHUNKS | KV_DEFER1)]
CHUNK_VALU = [CHUNK % KV_CHUNKS, CHUNK % (KV_CHUNKS | KV_DEAD1)]
# route_kernel<256, KV_UNIFORM | KV_PICKS | KV_DEFER1>: uniform layout, two or more dead shards
UNIFORM_DEFER1 = "_ZN3srk12route_kernelILi256ELj%dEEEvNS_11RouteParamsE" % (KV_PICKS | KV_DEFER1)
MFMA = "v_mfma_i32_16x16x64_i8"


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    if not os.path.exists(CO.LIB):
        pytest.fail(f"{CO.LIB} is not built")
    co = CO.extract(tmp_path_factory.mktemp("co"))
    if co is None:
        pytest.skip("llvm-objcopy / clang-offload-bundler not found")
    return co


@pytest.mark.parametrize("sym", CHUNK_MATRIX + CHUNK_VALU + [UNIFORM_DEFER1])
def test_seven_workgroups_per_cu_budget(code_object, sym):
    meta = CO.metadata(code_object)
    if meta is None:
        pytest.skip("llvm-readelf not found")
    assert sym in meta, f"{sym} is not in the library"
    m = meta[sym]
    print({k: m[k] for k in ("sgpr_count", "vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                             "sgpr_spill_count", "vgpr_spill_count")})
    assert m["vgpr_count"] <= 72
    assert m["sgpr_count"] <= 96
    assert m["group_segment_fixed_size"] <= 23040
    assert m["private_segment_fixed_size"] == 0
    assert m["vgpr_spill_count"] == 0


def test_which_kernels_hash_on_the_matrix_cores(code_object):
    counts = CO.instruction_counts(code_object, MFMA)
    if counts is None:
        pytest.skip("llvm-objdump not found")
    print({s: counts.get(s) for s in CHUNK_MATRIX + CHUNK_VALU + [UNIFORM_DEFER1]})
    for sym in CHUNK_MATRIX:
        assert counts.get(sym, 0) >= 8, sym
    for sym in CHUNK_VALU:
        assert sym in counts and counts[sym] == 0, sym
    assert counts.get(UNIFORM_DEFER1, 0) >= 8
