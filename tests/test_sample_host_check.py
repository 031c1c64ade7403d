"""The host part of the sample-rate stage (statsd-router_amd/csrc/sample_host.hpp: the parse that the count kernel
shares, the ladder, the keep rule, the rewrite, the configuration's check and the specs) under AddressSanitizer and
UndefinedBehaviorSanitizer: tools/sample_host_check.cpp, a stand-alone program with its own main over the header
alone, built with g++ and run once. Every line in it sits at the end of a heap block of exactly its size. Nothing
loaded into Python is built with a sanitizer."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_sample_host_check(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tools/sample_host_check.cpp")
    exe = str(tmp_path / "sample_host_check")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                            "-static-libubsan", "-o", exe,
                            os.path.join(REPO, "tools", "sample_host_check.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"


def test_sample_host_header_has_no_hip_call():
    """The header compiles without HIP: apart from the SRK_HD markers, no HIP header, type or call in it."""
    src = open(os.path.join(REPO, "statsd-router_amd", "csrc", "sample_host.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "#include <hip" not in code and "hipLaunch" not in code and "__global__" not in code
    assert "threadIdx" not in code and "__shared__" not in code and "__device__" not in code
