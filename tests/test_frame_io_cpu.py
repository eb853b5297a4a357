"""The per-frame I/O arithmetic of the extractor entries (ms-slam_amd/csrc/frame_io.h) on the CPU: tests/frame_io_main.cc, built
plain and with the address and undefined-behaviour sanitizers, one section per test.  block: the offsets of a frame's output
block for capacities 1, 2, 3, 657 and 2152, with and without the stereo fields, against the formulas written out in the test,
the regions disjoint and inside out_bytes, and the copy-out tail (both capacity messages, their order, every region).  planes:
the staging planes of msorb_extract_pair over every combination of `staged` bits and pointer positions (outside the block,
plane 0, plane 1, inside the block but not a plane start: refused)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-Wall", "-Werror", f"-I{ROOT}/ms-slam_amd/csrc", f"-I{ROOT}/include", f"{ROOT}/tests/frame_io_main.cc"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("frame_io") / f"frame_io_{request.param}"
    extra = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++"] + extra + FLAGS + ["-o", str(out)])
    return str(out)


@pytest.mark.parametrize("section", ["block", "planes"])
def test_section(exe, section):
    r = subprocess.run([exe, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"ok {section}" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
