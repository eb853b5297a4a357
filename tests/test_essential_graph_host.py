"""ms-slam_amd/csrc/essential_graph_device.h, the text the kernels compile, built for the host as tests/essential_graph_main.cc (g++ -O2,
and once under the address / undefined-behaviour sanitizers) and run serially over the GPU scenes against the forward restatement
of tests/essential_graph_cases.py: the counts equal, the estimates within 16 D and within 16 times the scene's own recorded spread.  tests/essential_graph_plan_main.cc checks the index
lists against a brute-force enumeration, plain and sanitized.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import essential_graph_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]
BUILDS = (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def _build(d, source):
    exes = {}
    for tag, extra in BUILDS:
        exes[tag] = str(d / f"{os.path.splitext(source)[0]}_{tag}")
        b = subprocess.run(["g++", *FLAGS, *extra, os.path.join(ROOT, "tests", source), "-o", exes[tag]], capture_output=True, text=True,
                           timeout=300)
        assert b.returncode == 0, b.stderr
    return exes


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("essential_graph_host")


@pytest.fixture(scope="module")
def mains(workdir):
    return _build(workdir, "essential_graph_main.cc")


@pytest.fixture(scope="module")
def plan_mains(workdir):
    return _build(workdir, "essential_graph_plan_main.cc")


def run_host(exe, workdir, tag, names):
    scenes = [ec.scene(n) for n in names]
    fin, fout = str(workdir / f"in_{tag}.bin"), str(workdir / f"out_{tag}.bin")
    ec.write_scenes(fin, scenes)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-3000:])
    return ec.read_results(fout, scenes)


def test_the_header_on_the_host_against_the_restatement(mains, workdir):
    bound, worst = ec.bound(), 0.0
    for name, r in zip(ec.GPU_SCENES, run_host(mains["plain"], workdir, "plain", ec.GPU_SCENES)):
        ref = ec.reference(name)
        dd = ec.estimate_difference(r["estimates"], ref["estimates"])
        worst = max(worst, dd)
        print(f"{name}: counts {ec.counts(r)} difference {dd:.3e} = {dd / ec.golden()['D']:.3f} D "
              f"chi2 {r['chi2_final']:.6e} (restatement {ref['chi2_final']:.6e})")
        assert ec.counts(r) == ec.counts(ref), name
        assert dd <= bound and dd <= ec.scene_bound(name), (name, dd, ec.scene_bound(name))
    print(f"largest host / restatement difference: {worst:.3e} = {worst / ec.golden()['D']:.3f} D (bound {ec.MARGIN} D)")


def test_the_header_under_the_sanitizers(mains, workdir):
    """every scene but the largest, whose dense factorisation takes a sanitized build half a minute"""
    names = [n for n in ec.GPU_SCENES if n != "free150_loops"]
    for name, r in zip(names, run_host(mains["sanitized"], workdir, "sanitized", names)):
        assert ec.counts(r) == ec.counts(ec.reference(name)), name


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_the_plan_against_brute_force(plan_mains, workdir, build):
    for name in ec.GPU_SCENES:
        sc = ec.scene(name)
        path = str(workdir / f"plan_{build}_{name}.bin")
        with open(path, "wb") as f:
            f.write(np.array([len(sc["fixed"]), len(sc["v0"])], np.int32).tobytes())
            for k in ("fixed", "v0", "v1"):
                f.write(np.ascontiguousarray(sc[k], np.int32).tobytes())
        p = subprocess.run([plan_mains[build], path], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.rstrip().endswith("ok"), (name, p.stdout[-600:], p.stderr[-2000:])
        print(name, p.stdout.splitlines()[0])
