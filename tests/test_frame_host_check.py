"""The host arithmetic of device framing (statsd-router_amd/csrc/frame_host.hpp, host/sr_slots.h) under
AddressSanitizer and UndefinedBehaviorSanitizer: tools/frame_host_check.cpp, a stand-alone program with its own main over the
headers alone, built with g++ and run once. It checks the framed total and ends of slot arenas that end with
their last kept byte (lengths at every edge of the 4095-byte cap, with and without a final '\\n', strides
4096 to 70000) and the offset-to-datagram search at every datagram's first and last framed byte, across
runs of empty datagrams. Nothing loaded into Python is built with a sanitizer."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_frame_host_check(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tools/frame_host_check.cpp")
    exe = str(tmp_path / "frame_host_check")
    # the sanitizer runtimes linked into the program itself: it then runs the same whatever else the
    # process environment loads ahead of it
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                            "-static-libubsan", "-o", exe,
                            os.path.join(REPO, "tools", "frame_host_check.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"


def test_frame_host_header_has_no_hip():
    """The header compiles without HIP: no HIP header, type or call in it."""
    src = open(os.path.join(REPO, "statsd-router_amd", "csrc", "frame_host.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "hip" not in code.lower()
