"""The rendezvous board of the in-process communicator (statsd-router_amd/csrc/local_board.hpp) on the CPU:
tools/local_board_check.cpp, a stand-alone program over the header alone with a fake device, built with
plain g++ and run once. It checks 2, 3 and 8 threads through 200 rounds of all-pairs messages under three
tags (matching order, payload identity, one pull per group, no wait for an event that is not recorded), a
rank without operations, a size mismatch, and an absent peer (-ETIMEDOUT after the deadline and not before,
then -EPIPE at once for the latecomer)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_local_board_check(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tools/local_board_check.cpp")
    exe = str(tmp_path / "local_board_check")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Wextra", "-Werror", "-o", exe,
                            os.path.join(REPO, "tools", "local_board_check.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"


def test_board_header_has_no_hip():
    """The board compiles without HIP: no HIP header, type or call in it."""
    src = open(os.path.join(REPO, "statsd-router_amd", "csrc", "local_board.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "hip" not in code.lower()
