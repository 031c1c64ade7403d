"""The gfx950 code object inside the built libsr_route.so, for the tests that read the kernels' budgets
and instructions without a GPU: its metadata ({kernel symbol: {key: int}}) and its disassembly per
kernel. A plain helper module (no fixtures); callers skip when a tool is missing."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "statsd-router_amd", "lib", "libsr_route.so")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def tool(name):
    """Path of an LLVM tool of the ROCm installation (or of PATH), or None."""
    for d in [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"]:
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def extract(tmpdir, lib=LIB):
    """Unbundle the library's gfx950 code object into tmpdir; returns its path, or None when
    llvm-objcopy or clang-offload-bundler is missing."""
    objcopy, bundler = tool("llvm-objcopy"), tool("clang-offload-bundler")
    if not objcopy or not bundler:
        return None
    fatbin, co = os.path.join(str(tmpdir), "fatbin"), os.path.join(str(tmpdir), "gfx950.co")
    subprocess.run([objcopy, f"--dump-section=.hip_fatbin={fatbin}", lib, os.path.join(str(tmpdir), "rest")],
                   check=True, capture_output=True)
    subprocess.run([bundler, "--unbundle", "--type=o", f"--input={fatbin}", f"--output={co}",
                    f"--targets={TARGET}"], check=True, capture_output=True)
    return co


def metadata(co):
    """{kernel symbol: {metadata key: int}} from the code object's notes, or None without llvm-readelf."""
    readelf = tool("llvm-readelf")
    if not readelf:
        return None
    notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
    meta = {}
    for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return meta


def instruction_counts(co, mnemonic):
    """{function symbol: occurrences of `mnemonic`} from llvm-objdump -d, or None without the tool."""
    objdump = tool("llvm-objdump")
    if not objdump:
        return None
    text = subprocess.run([objdump, "-d", co], check=True, capture_output=True, text=True).stdout
    counts, cur = {}, None
    pat = re.compile(r"\b" + re.escape(mnemonic) + r"\b")
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
            counts[cur] = 0
        elif cur is not None and pat.search(line):
            counts[cur] += 1
    return counts
