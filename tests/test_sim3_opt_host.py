"""ms-slam_amd/csrc/sim3_opt_device.h, the text the kernel compiles, built for the host as tests/sim3_opt_main.cc (plain, and under the
address / undefined-behaviour sanitizers) and run serially in forward order over the GPU scenes, against the forward restatement
of tests/sim3_opt_cases.py under the device's bounds.  On the glibc this was written on it is bit-equal, which the test prints
and does not require.  No GPU, nothing loaded into Python."""
import json
import os
import subprocess

import numpy as np
import pytest

import sim3_opt_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mains(tmp_path_factory):
    d = tmp_path_factory.mktemp("sim3_opt_main")
    src = os.path.join(ROOT, "tests", "sim3_opt_main.cc")
    flags = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]
    exes = {}
    for tag, extra in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[tag] = str(d / tag)
        b = subprocess.run(["g++", *flags, *extra, src, "-o", exes[tag]], capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr
    return d, exes


@pytest.fixture(scope="module")
def golden():
    with open(sc.GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("one_step", [False, True], ids=["full", "one_step"])
@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_the_header_on_the_host_against_the_restatement(mains, golden, build, one_step):
    d, exes = mains
    names = list(sc.ONE_STEP if one_step else sc.GPU_SCENES)
    scenes = [sc.scene(n) for n in names]
    fin, fout = str(d / f"in_{build}_{one_step}.bin"), str(d / f"out_{build}_{one_step}.bin")
    sc.write_problems(fin, scenes, (1, 1, 1) if one_step else sc.ITS)
    p = subprocess.run([exes[build], fin, fout], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-3000:])
    g = golden["one_step"] if one_step else golden
    bit_equal = 0
    for name, s, r in zip(names, scenes, sc.read_results(fout, scenes)):
        ref = sc.reference(name, one_step=one_step)
        dd = sc.estimate_difference(r, ref, s["median_depth"])
        cc = sc.chi2_difference(r["chi2"], ref["chi2"], ref["th2"])
        same = (r["q"].tobytes() == ref["q"].tobytes() and r["t"].tobytes() == ref["t"].tobytes() and r["s"] == ref["s"]
                and np.array_equal(r["chi2"], ref["chi2"], equal_nan=True))
        bit_equal += same
        print(f"{name}: D={dd:.3e} C={cc:.3e} bit_equal={same}")
        assert np.array_equal(r["bad"], ref["bad"]), name
        assert (r["status"], r["n_pairs"], r["n_bad"], r["n_in"]) == (ref["status"], ref["n_pairs"], ref["n_bad"], ref["n_in"]), name
        assert dd <= g["estimate_bound"] and cc <= g["chi2_bound"], name
        if sc.variants_agree(name, one_step):
            assert r["iterations"] == ref["iterations"] and r["rejected_trials"] == ref["rejected_trials"], name
        else:
            assert [v >= 0 for v in r["iterations"]] == [v >= 0 for v in ref["iterations"]], name
    print(f"bit-equal with the forward restatement: {bit_equal} of {len(names)} scenes")
