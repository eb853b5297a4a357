"""The claim replay of ms-slam_amd/csrc/claim_replay.h (the sequential accept rule of the SearchByProjection forms over device lists
ranked against an occupancy snapshot) on the CPU: tests/claim_replay_main.cc plays the device itself and compares matches, final
occupancy and match count with the reference's sequential loop on drawn scenes — one side with the ratio rule and with the
distance threshold, two cameras with partner claims, each also with queries built on the device (windows unknown to the replay).
The program counts in how many scenes a list was exhausted, a keypoint freed, a side changed by the other camera before its first
query, and fails below 10 % each.  Compiled with g++ against the two HIP-free headers, once plain and once under the address and
undefined-behaviour sanitizers; no hipcc, no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "claim_replay_main.cc")
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", f"-I{ROOT}/ms-slam_amd/csrc"]


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_claim_replay_equals_the_sequential_loop(tmp_path, sanitize):
    exe = str(tmp_path / "claim_replay")
    b = subprocess.run(["g++", *FLAGS, *sanitize, MAIN, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout)   # the coverage shares per form
    assert p.returncode == 0, f"exit status {p.returncode}\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "ok" and len(lines) == 7, p.stdout
