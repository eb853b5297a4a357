"""ms-slam_amd/csrc/bow_pairs.h (the plain C++ of the BoW-node searches: the merge walk over two FeatureVectors, the order-free
rotation filter, the candidate pick of the search with a caller's predicate, the camera split of a two-camera frame's vector, the
packing of the triangulation side) on the CPU: tests/bow_pairs_main.cc compares each with a restatement of the reference's loops
written in that program — the visiting-order histogram of 30 vectors, the running-minimum scan — on drawn inputs, counts how often
the cases that make a rule bite occur (bins that tie, maxima dropped by the 0.1 rule, the wrap of bin 30, NaN angles, equal
distances, claimed or refused best candidates, ...) and fails below 10 % each.  Compiled with g++ against the HIP-free headers,
once plain and once under the address and undefined-behaviour sanitizers; no hipcc, no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "bow_pairs_main.cc")
FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", f"-I{ROOT}/ms-slam_amd/csrc"]


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_bow_pairs_equal_the_restated_loops(tmp_path, sanitize):
    exe = str(tmp_path / "bow_pairs")
    b = subprocess.run(["g++", *FLAGS, *sanitize, MAIN, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout)   # the coverage shares
    assert p.returncode == 0, f"exit status {p.returncode}\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "ok" and len(lines) == 14, p.stdout
