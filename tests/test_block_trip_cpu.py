"""BlockLayout and round_trip of ms-slam_amd/csrc/block_trip.h (the staged block and the stream chain of the BoW-node searches) on the
CPU: tests/block_trip_main.cc, compiled with g++ against the HIP stand-in of tests/hip_stub, checks the region offsets, the order
of the stream operations with and without timing events, what a trip moves, and that a failed launch names the entry and releases
the thread's scratch.  Plain and under the address / undefined-behaviour sanitizers; no hipcc, no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "block_trip_main.cc")
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", f"-I{ROOT}/tests/hip_stub", f"-I{ROOT}/ms-slam_amd/csrc"]


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_round_trip_order_and_failure(tmp_path, sanitize):
    exe = str(tmp_path / "block_trip")
    b = subprocess.run(["g++", *FLAGS, *sanitize, MAIN, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"exit status {p.returncode}\n{p.stderr[-4000:]}"
    assert p.stdout.strip() == "ok", p.stdout
