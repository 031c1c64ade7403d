"""The three framing kernels (statsd-router_amd/csrc/frame_kernel.hpp) in the built library's code-object
metadata (no GPU needed): each is there, uses no scratch and spills no VGPR, and the gather stays within what
lets eight of its 256-thread workgroups share a CU (64 VGPRs, 20 KiB of LDS)."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO

LIB = os.path.join(REPO, "statsd-router_amd", "lib", "libsr_route.so")
FRAME_KERNELS = {
    "_ZN3srk17frame_lens_kernelENS_9FrameArgsE": 1024,
    "_ZN3srk17frame_scan_kernelENS_9FrameArgsE": 64,
    "_ZN3srk19frame_gather_kernelENS_9FrameArgsE": 256,
}


def _tool(name):
    for d in [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"]:
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


@pytest.fixture(scope="module")
def kernel_meta(tmp_path_factory):
    """{kernel symbol: {metadata key: int}} of the gfx950 code object inside libsr_route.so."""
    objcopy, bundler, readelf = _tool("llvm-objcopy"), _tool("clang-offload-bundler"), _tool("llvm-readelf")
    if not objcopy or not bundler or not readelf:
        pytest.skip("llvm-objcopy / clang-offload-bundler / llvm-readelf not found")
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} is not built")
    tmp = tmp_path_factory.mktemp("co")
    fatbin, co = str(tmp / "fatbin"), str(tmp / "gfx950.co")
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fatbin}", LIB, str(tmp / "rest")], check=True,
                   capture_output=True)
    subprocess.run([bundler, "--unbundle", "--type=o", f"--input={fatbin}", f"--output={co}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True, capture_output=True)
    notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
    meta = {}
    for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    assert meta, "no kernel metadata in the code object"
    return meta


@pytest.mark.parametrize("sym", sorted(FRAME_KERNELS))
def test_frame_kernels_use_no_scratch(kernel_meta, sym):
    assert sym in kernel_meta, f"{sym} is not in the library"
    m = kernel_meta[sym]
    print({k: m[k] for k in ("sgpr_count", "vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                             "sgpr_spill_count", "vgpr_spill_count")})
    assert m["private_segment_fixed_size"] == 0
    assert m["vgpr_spill_count"] == 0
    assert m["max_flat_workgroup_size"] == FRAME_KERNELS[sym]


def test_gather_fits_eight_workgroups_per_cu(kernel_meta):
    m = kernel_meta["_ZN3srk19frame_gather_kernelENS_9FrameArgsE"]
    assert m["vgpr_count"] <= 64 and m["sgpr_count"] <= 80 and m["group_segment_fixed_size"] <= 20480


def test_frame_kernel_names_leave_the_route_kernel_set_alone():
    """tests/test_abi.py pins the library's route_kernel< / route_chunk_kernel< instantiations by name."""
    assert not any("route_kernel" in s or "route_chunk_kernel" in s for s in FRAME_KERNELS)
