"""ms-slam_amd/csrc/inertial_device.h, the text the kernel compiles, and inertial_plan.h built for the host as
tests/inertial_opt_main.cc (g++ -O2, and once under the address / undefined-behaviour sanitizers: a stand-alone program, nothing
loaded into Python) and run serially over the GPU scenes against the forward restatement of tests/inertial_opt_cases.py: status and
the number of active edges equal, the counts equal where the golden file says the variants agree, every estimate and every edge's
chi2 within 16 D.  Bit-equality with the restatement is printed, not required.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import inertial_opt_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]
BUILDS = (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("inertial_opt_host")


@pytest.fixture(scope="module")
def mains(workdir):
    exes = {}
    for tag, extra in BUILDS:
        exes[tag] = str(workdir / f"inertial_opt_main_{tag}")
        b = subprocess.run(["g++", *FLAGS, *extra, os.path.join(ROOT, "tests", "inertial_opt_main.cc"), "-o", exes[tag]],
                           capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr
    return exes


def run_host(exe, workdir, tag, names):
    scenes = [ic.scene(n) for n in names]
    fin, fout = str(workdir / f"in_{tag}.bin"), str(workdir / f"out_{tag}.bin")
    ic.write_scenes(fin, scenes)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-3000:])
    return ic.read_results(fout, scenes)


def check(name, r, ref, what):
    g, b = ic.golden(), ic.bounds()
    d = ic.differences(r, ref, ic.scene(name)["truth"]["speed"])
    same = all(np.array_equal(r[k], ref[k]) for k in ("v", "bg", "ba", "Rwg", "chi2")) and r["scale"] == ref["scale"]
    print(f"{name}: {what} counts {ic.counts(r)} restatement {ic.counts(ref)} bit-equal {same} in D: "
          + " ".join(f"{q} {d[q] / g['D'][q]:.3f}" for q in ic.QUANTITIES if g["D"][q] > 0))
    assert (r["status"], r["n_active_edges"]) == (ref["status"], ref["n_active_edges"]), name
    if g["scenes"][name]["counts_agree"]:
        assert ic.counts(r) == ic.counts(ref), name
    if ic.counts(r) == ic.counts(ref):                            # a run of another length is another computation
        assert ic.within(d, b), (name, d, b)
    return d


def test_the_header_on_the_host_against_the_restatement(mains, workdir):
    worst = {q: 0.0 for q in ic.QUANTITIES}
    for name, r in zip(ic.GPU_SCENES, run_host(mains["plain"], workdir, "plain", ic.GPU_SCENES)):
        d = check(name, r, ic.reference(name), "host")
        worst = {q: max(worst[q], d[q]) for q in ic.QUANTITIES}
        K = len(ic.scene(name)["kfs"])
        lonely = np.setdiff1d(np.arange(K), ic.chains(ic.scene(name))[0])
        assert r["v"][lonely].tobytes() == ic.scene(name)["kfs"]["v"][lonely].tobytes()
    D = ic.golden()["D"]
    print("largest host / restatement difference in D:", {q: worst[q] / D[q] for q in ic.QUANTITIES if D[q] > 0}, "bound", ic.MARGIN)


def test_the_header_under_the_sanitizers(mains, workdir):
    names = [n for n in ic.GPU_SCENES if len(ic.scene(n)["kfs"]) <= 300]
    for name, r in zip(names, run_host(mains["sanitized"], workdir, "sanitized", names)):
        ref = ic.reference(name)
        assert (r["status"], r["n_active_edges"]) == (ref["status"], ref["n_active_edges"]), name


def test_the_plan_refuses_malformed_structures(mains, workdir):
    cases = [(4, [0, 1, 2], [1, 2, 3], 0, 4),      # a chain
             (5, [0, 3], [1, 4], 0, 4),            # two chains and a KeyFrame without an edge
             (4, [0, 0], [1, 2], 2, 0),            # a fork: two outgoing edges
             (4, [0, 2], [1, 1], 2, 0),            # two incoming edges
             (3, [0, 1, 2], [1, 2, 0], 3, 0),      # a cycle
             (5, [0, 2, 3], [1, 3, 2], 3, 0),      # a chain and a cycle of two
             (3, [0, 1], [1, 3], 1, 0),            # an index out of range
             (3, [-1], [1], 1, 0),
             (3, [1], [1], 1, 0),                  # an edge from a KeyFrame to itself
             (0, [], [], 0, 0)]
    path = str(workdir / "plans.bin")
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for K, prev, cur, _, _ in cases:
            f.write(np.array([K, len(prev)], np.int32).tobytes() + np.array(prev, np.int32).tobytes() + np.array(cur, np.int32).tobytes())
    for tag in ("plain", "sanitized"):
        p = subprocess.run([mains[tag], "--plans", path], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr[-2000:]
        got = [tuple(int(x) for x in line.split()) for line in p.stdout.strip().splitlines()]
        assert got == [(c[3], c[4]) for c in cases], (tag, got)
