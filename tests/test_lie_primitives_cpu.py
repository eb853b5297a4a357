"""The shared Lie-group primitives of the optimisers, one function at a time, on the host: ms-slam_amd/csrc/lie_probe_device.h (the
text msorb_debug_lie compiles, which calls se3_device.h, sim3_opt_device.h, essential_graph_device.h, essential_graph4_device.h,
inertial_device.h and mlpnp_device.h) built as tests/lie_probe_main.cc with g++ -O2, and once under the address / undefined-behaviour
sanitizers (a stand-alone program, nothing loaded into Python), and run over every record of tests/lie_primitives_cases.py:

 - the condition on the inputs: no record sits where the exact value (the reference's formula in mpmath) and a float run take
   different branches; the only records on a predicate are those whose predicate is decided in exact arithmetic;
 - the host program within 16 D(function, family) of the exact value, D from tests/golden/lie_primitives_sensitivity.json;
 - on the libm-free functions and arms, the host program equal, bit for bit, to the float restatements of the same statement;
 - the golden file reproduced from scratch.
No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import lie_primitives_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]
BUILDS = (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


@pytest.fixture(scope="module")
def host_outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("lie_primitives_cpu")
    blocks = [(fn, lc.records(fn)[0]) for fn in lc.OPS] + [("se3_exp", np.zeros((0, lc.LIE_IN)))]   # (an empty block is valid)
    lc.write_blocks(str(d / "in.bin"), blocks)
    out = {}
    for tag, extra in BUILDS:
        exe = str(d / f"lie_probe_main_{tag}")
        b = subprocess.run(["g++", *FLAGS, *extra, os.path.join(ROOT, "tests", "lie_probe_main.cc"), "-o", exe], capture_output=True,
                           text=True, timeout=600)
        assert b.returncode == 0, b.stderr
        p = subprocess.run([exe, str(d / "in.bin"), str(d / f"out_{tag}.bin")], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (tag, p.stdout[-400:], p.stderr[-3000:])
        out[tag] = dict(zip(lc.OPS, lc.read_blocks(str(d / f"out_{tag}.bin"), blocks)))
    return out


@pytest.mark.parametrize("fn", lc.OPS)
def test_no_record_sits_on_a_branch(fn):
    rec, fams, decided = lc.records(fn)
    assert len(rec) >= 40 and rec.shape[1] == lc.in_width(fn)
    if fn in lc.FLOAT_CHAIN:                                      # float functions take exactly representable floats
        k = 66 if fn == "bias_corrected" else 9
        assert np.array_equal(rec[:, :k], rec[:, :k].astype(np.float32).astype(np.float64))
    bad = lc.condition_violations(fn)
    assert not bad, (len(bad), [(i, fams[i], what) for i, what in bad[:5]])


@pytest.mark.parametrize("fn", lc.OPS)
def test_the_golden_record_is_current(fn):
    g, m = lc.golden()[fn], lc.measure(fn)
    assert sorted(g) == sorted(m) == sorted(set(lc.records(fn)[1]))
    for fam in m:
        assert math.isclose(g[fam], m[fam], rel_tol=1e-6, abs_tol=0.0), (fn, fam, g[fam], m[fam])


@pytest.mark.parametrize("fn", lc.OPS)
def test_the_host_program_against_the_exact_value(fn, host_outputs):
    out = host_outputs["plain"][fn]
    worst, _, _, failures = lc.judge(fn, out)
    print(f"{fn}: {len(out)} records, host program: largest distance / D {worst:.3f}")
    assert not failures, (len(failures), failures[:5])
    bad = lc.statement_mismatches(fn, out)
    assert not bad, (len(bad), bad[:5])


def test_the_branches_the_scenes_never_enter_are_entered():
    """the records reach what the optimisers' scenes do not: the three else arms of quaternion_of_matrix, all four (sigma, theta)
    branches of Sim3's exponential and logarithm, the three exits of LogSO3, both arms of every 1e-5 threshold"""
    def outcomes(fn):
        return {(tag, r) for t in lc.exact(fn)[1] for tag, r in t}
    arms = set()
    for t in lc.exact("quaternion_of_matrix")[1]:
        d = dict(t)
        if not d["trace>0"]:
            arms.add(2 if d["R22>Rii"] else (1 if d["R11>R00"] else 0))
    assert arms == {0, 1, 2}
    for fn, tags in (("se3_exp", ("theta<1e-5", "trace>0", "qw<0")), ("sim3_exp", ("theta<1e-5", "|sigma|<1e-5", "trace>0")),
                     ("sim3_log", ("d>1-eps", "|sigma|<1e-5", "pivot")), ("exp_so3", ("d<1e-5",)), ("right_jacobian_so3", ("d<1e-5",)),
                     ("inverse_right_jacobian_so3", ("d<1e-5",)), ("so3f_exp_matrix", ("theta_sq<eps^2",)), ("log_so3", ("cos>1", "cos<-1", "|sin|<1e-5")),
                     ("mlpnp_rodrigues2rot", ("th>eps",)), ("mlpnp_rot2rodrigues", ("wnorm>eps",)), ("huber", ("chi2<=dsqr",)),
                     ("bias_corrected", ("theta_sq<eps^2",)), ("lu3_solve", ("pivot",)), ("normalize_rotation", ("qw<0",))):
        o = outcomes(fn)
        for tag in tags:
            assert (tag, True) in o and (tag, False) in o, (fn, tag)
    for fn in ("sim3_exp", "sim3_log"):                              # all four (sigma, theta) combinations
        small = "theta<1e-5" if fn == "sim3_exp" else "d>1-eps"
        assert {(dict(t)[small], dict(t)["|sigma|<1e-5"]) for t in lc.exact(fn)[1]} == {(a, b) for a in (False, True) for b in (False, True)}
    nan = [i for i, v in enumerate(lc.exact("mlpnp_rot2rodrigues")[0]) if lc.records("mlpnp_rot2rodrigues")[0][i][0] > 1.0]
    assert nan and all(all(c == 0 for c in lc.exact("mlpnp_rot2rodrigues")[0][i]) for i in nan)   # acos above 1: w = 0


def test_the_sanitized_build_returns_the_same_bits(host_outputs):
    """the unrolled index arithmetic of quaternion_of_matrix and lu3_solve's permutation on the edge records, under ASan / UBSan"""
    for fn in lc.OPS:
        a, b = host_outputs["plain"][fn], host_outputs["sanitized"][fn]
        assert a.tobytes() == b.tobytes() or np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]), fn
