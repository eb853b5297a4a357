"""ms-slam_amd/csrc/mlpnp_device.h and mlpnp_select.h, the text the kernels compile, built for the host as tests/mlpnp_main.cc (plain,
and under the address / undefined-behaviour sanitizers) and run directly, against R64 of tests/mlpnp_cases.py: every hypothesis'
pose within 16 D, counts, flags, winner record and mask equal.  D is the largest spread of a finite hypothesis pose among the
variants of tests/mlpnp_cases.py (other summation orders, another nullspace basis, LAPACK in place of the Jacobi iterations, libm
one ulp off), measured by running that module as a script and recorded in tests/golden/mlpnp_ransac_spread.json; 16 D is the
project's margin of DESIGN.md sections 9 and 10.  On the glibc this was written on the program is bit-equal to R64, which the
test prints and does not require.  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import mlpnp_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mains(tmp_path_factory):
    d = tmp_path_factory.mktemp("mlpnp_main")
    src = os.path.join(ROOT, "tests", "mlpnp_main.cc")
    flags = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]
    exes = {}
    for tag, extra in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[tag] = str(d / tag)
        b = subprocess.run(["g++", *flags, *extra, src, "-o", exes[tag]], capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr
    return d, exes


def _run(mains, build, mode, payload, tag):
    d, exes = mains
    fin, fout = str(d / f"{tag}_{build}.in"), str(d / f"{tag}_{build}.out")
    if isinstance(payload, bytes):
        with open(fin, "wb") as f:
            f.write(payload)
    else:
        mc.write_problems(fin, payload)
    p = subprocess.run([exes[build], mode, fin, fout], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-3000:])
    return fout


def test_scene_list_covers_what_it_names():
    admitted = mc.admitted()
    assert set(mc.EDGE) <= set(admitted) and len(mc.GENERATED) - len([n for n in mc.GENERATED if n in admitted]) <= len(mc.GENERATED) // 10
    runs = {n: mc.prepared(n) for n in admitted}
    assert {6, 7, 63, 64, 65, 257} <= {len(sc["p2d"]) for sc, _ in runs.values()}
    assert {1, 35, 300} <= {len(sc["sets"]) for sc, _ in runs.values()}
    sc, r = runs["n=6,set=all"]
    assert sorted(sc["sets"][0]) == list(range(6)) and r["counts"][0] == 6
    sc, r = runs["plane,range=3"]                      # Gauss-Newton recovers the mis-scaled translation on clean sets
    assert (r["flags"] & mc.PLANAR).all() and (r["counts"] >= 48).all() and (r["counts"] == 64).sum() > 17
    sc, r = runs["plane,range=12"]                     # the first step exceeds 5: the break, no update, no inlier
    assert (r["flags"] == (mc.PLANAR | mc.BROKE)).all() and not r["counts"].any() and r["winner"] == -1
    sc, r = runs["all outliers"]
    assert r["winner"] == -1 and not r["inliers"].any() and r["consumed"] == 35
    sc, r = runs["behind"]                             # no depth test: the points behind the camera are the winner's inliers
    assert r["winner"] >= 0 and r["inliers"][[3, 9, 20]].all()
    sc, r = runs["repeated point"]
    assert np.array_equal(sc["p3d"][0], sc["p3d"][1]) and {0, 1} <= set(sc["sets"][0])
    sc, r = runs["count==min"]
    first = int(np.argmax(r["counts"]))
    assert r["counts"][first] == sc["min_inliers"] and not r["converged"] and r["winner"] == first and r["consumed"] == 35
    sc, r = runs["carried best"]
    assert r["converged"] and r["best_h"] == -1 and r["counts"][r["winner"]] < sc["best_inliers_in"]
    assert r["winner"] != int(np.argmax(r["counts"]))   # handed out although it is not the best
    assert any(r["converged"] and r["winner"] > 0 for _, r in runs.values())
    sc, r = runs["non-finite"]
    assert not np.isfinite(r["poses"][0]).all() and r["counts"][0] == 0 and r["winner"] > 0 and not r["masks"][:, 4].any()


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_the_header_on_the_host_against_r64(mains, build):
    names = mc.admitted()
    prep = [mc.prepared(n) for n in names]
    fout = _run(mains, build, "run", [sc for sc, _ in prep], "run")
    bound, bit_equal = 16 * mc.load_spread(), 0
    for name, (sc, ref), r in zip(names, prep, mc.read_results(fout, [sc for sc, _ in prep])):
        d, _ = mc.pose_difference(r["poses"], ref["poses"])
        same_bits = r["poses"].tobytes() == ref["poses"].tobytes()
        bit_equal += same_bits
        print(f"{name}: pose difference {d:.3e} (bound {bound:.3e}) bit_equal={same_bits}")
        assert mc.same(r, ref, bound) is None, (name, mc.same(r, ref, bound))
    print(f"bit-equal with R64: {bit_equal} of {len(names)} scenes")


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_the_selection_rule_against_a_plain_loop(mains, build):
    rng = np.random.RandomState(5)
    cases = []
    for k in range(400):
        n = int(rng.randint(1, 40))
        mn = int(rng.randint(0, 12))
        counts = rng.randint(0, 14, n).astype(np.int32)
        kind = k % 4
        if kind == 1:      # count == min exists and nothing above it
            counts = np.minimum(counts, mn).astype(np.int32)
            counts[rng.randint(n)] = mn
        if kind == 2:      # nothing reaches min
            counts = np.minimum(counts, max(mn - 1, 0)).astype(np.int32)
            mn = max(mn, 1)
        best = int(rng.randint(0, 16)) if kind == 3 else 0     # a carried best
        cases.append((n, mn, best, counts))
    payload = np.int32(len(cases)).tobytes() + b"".join(np.array([n, mn, best], np.int32).tobytes() + c.tobytes() for n, mn, best, c in cases)
    out = np.fromfile(_run(mains, build, "select", payload, "select"), np.int32).reshape(-1, 5)
    seen = set()
    for (n, mn, best, counts), o in zip(cases, out):
        s = mc.select(counts, mn, best)
        assert tuple(o) == (s["winner"], s["converged"], s["consumed"], s["best"], s["best_h"]), (n, mn, best, counts)
        seen.add((s["converged"], s["winner"] >= 0, s["converged"] and s["best_h"] != s["winner"]))
    assert {(1, True, False), (1, True, True), (0, True, False), (0, False, False)} <= seen


def test_the_jacobian_against_central_differences(mains):
    """h = 1e-6 on values of order 1: the truncation error of a central difference is h^2 = 1e-12 of the third derivative, the
    rounding error eps / h = 2e-10 of the residual (|r| <= 1, the entries are of order 0.1-1), so 1e-8 of the largest entry holds
    both with a margin of ten or more."""
    rng = np.random.RandomState(9)
    h = 1e-6
    rows = []
    for _ in range(40):
        w = rng.normal(size=3) * rng.uniform(0.05, 1.5)
        T = rng.uniform(-1, 1, 3)
        p = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(4, 12)])
        f = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), 1.0])
        n = np.cross(f, rng.normal(size=3))
        n /= np.linalg.norm(n)
        x = np.concatenate([w, T])
        rows.append(np.concatenate([x, p, n]))
        for k in range(6):
            for sgn in (1, -1):
                xx = x.copy()
                xx[k] += sgn * h
                rows.append(np.concatenate([xx, p, n]))
    rows.append(np.concatenate([np.zeros(3), [0.1, 0.2, 0.3], [1.0, 2.0, 8.0], [1.0, 0.0, 0.0]]))     # w = 0
    rows = np.array(rows)
    payload = np.int32(len(rows)).tobytes() + rows.tobytes()
    out = np.fromfile(_run(mains, "plain", "jac", payload, "jac"), np.float64).reshape(-1, 7)
    worst = 0.0
    for c in range(40):
        blk = out[13 * c:13 * c + 13]
        J = blk[0, 1:]
        num = np.array([(blk[1 + 2 * k, 0] - blk[2 + 2 * k, 0]) / (((rows[13 * c + 1 + 2 * k, k]) - (rows[13 * c + 2 + 2 * k, k]))) for k in range(6)])
        err = np.abs(J - num).max() / np.abs(J).max()
        worst = max(worst, err)
        assert err <= 1e-8, (c, J, num)
        # the restatement's Jacobian is the header's, operation for operation
        v = rows[13 * c]
        pose = mc._Pose(mc.Variant())
        r64, J64 = pose.residual_and_jacobian(pose.rodrigues2rot(v[:3]), v[:3], v[3:6], v[6:9], v[9:12])
        assert np.abs(J64 - J).max() <= 16 * mc.load_spread() and abs(r64 - blk[0, 0]) <= 16 * mc.load_spread()
    print(f"largest |J - central difference| / max|J|: {worst:.3e}")
    assert not np.isfinite(out[-1, 1:4]).any()           # non-finite at w = 0, as the reference's expression is
