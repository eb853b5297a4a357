"""ms-slam_amd/csrc/essential_graph4_device.h, the text the kernels compile, built for the host as tests/essential_graph4_main.cc
(g++ -O2, and once under the address / undefined-behaviour sanitizers: a stand-alone program, nothing loaded into Python) and run
serially over the GPU scenes against the forward restatement of tests/essential_graph4_cases.py: the counts equal, lambda_initial
within 16 D relative, the poses within 16 D and within 16 times the scene's own recorded spread.  No GPU."""
import os
import subprocess

import pytest

import essential_graph4_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]
BUILDS = (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("essential_graph4_host")


@pytest.fixture(scope="module")
def mains(workdir):
    exes = {}
    for tag, extra in BUILDS:
        exes[tag] = str(workdir / f"essential_graph4_main_{tag}")
        b = subprocess.run(["g++", *FLAGS, *extra, os.path.join(ROOT, "tests", "essential_graph4_main.cc"), "-o", exes[tag]],
                           capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr
    return exes


def run_host(exe, workdir, tag, names):
    scenes = [ec.scene(n) for n in names]
    fin, fout = str(workdir / f"in_{tag}.bin"), str(workdir / f"out_{tag}.bin")
    ec.write_scenes(fin, scenes)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-3000:])
    return ec.read_results(fout, scenes)


def test_the_header_on_the_host_against_the_restatement(mains, workdir):
    bound, worst, D = ec.bound(), 0.0, ec.golden()["D"]
    for name, r in zip(ec.GPU_SCENES, run_host(mains["plain"], workdir, "plain", ec.GPU_SCENES)):
        ref = ec.reference(name)
        dd = ec.pose_difference(r["poses"], ref["poses"])
        worst = max(worst, dd)
        print(f"{name}: counts {ec.counts(r)} difference {dd:.3e} = {dd / D:.3f} D = "
              f"{dd / max(ec.golden()['scenes'][name]['spread'], 2.3e-16):.3f} own spreads; lambda_initial {r['lambda_initial']:.9e} "
              f"(restatement {ref['lambda_initial']:.9e}); chi2 {r['chi2_final']:.6e} (restatement {ref['chi2_final']:.6e})")
        assert ec.counts(r) == ec.counts(ref), name
        assert ec.lambda_agrees(r["lambda_initial"], ref["lambda_initial"]), name
        assert dd <= bound and dd <= ec.scene_bound(name), (name, dd, ec.scene_bound(name))
    print(f"largest host / restatement difference: {worst:.3e} = {worst / D:.3f} D (bound {ec.MARGIN} D)")


def test_the_header_under_the_sanitizers(mains, workdir):
    """every scene but the largest, whose dense factorisation takes a sanitized build several seconds"""
    names = [n for n in ec.GPU_SCENES if n != "free150_loops"]
    for name, r in zip(names, run_host(mains["sanitized"], workdir, "sanitized", names)):
        assert ec.counts(r) == ec.counts(ec.reference(name)), name
