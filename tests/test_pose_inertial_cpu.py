"""tests/pose_inertial_cases.py, the numpy restatement of Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame, and
ms-slam_amd/csrc/pose_inertial_device.h compiled for the host (tests/pose_inertial_main.cc, once more under AddressSanitizer and
UBSan): the host program against the forward restatement, the committed sensitivity file measured again, the conditions that make
"flags equal" a fair demand, what each scene was built to show, the analytic Jacobians of the restated edges against central
differences, the generator's state recovered on noise-free scenes, and Marginalize against the Schur complement.  No GPU, no library.

Bounds.  D is, per quantity (the entries of Rwb, twb over the median depth, the velocity over the speed, bg, ba, every compared
chi2 relative to max(chi2, threshold), H_raw and H_prior relative to their largest entry), the largest difference between the
forward restatement and any of its variants over the GPU scenes: tests/golden/pose_inertial_sensitivity.json.  Another statement of
the same arithmetic may differ from the restatement by 16 D (DESIGN.md sections 9 to 20); flags, counts and round lengths are equal.
The C ABI returns no per-edge chi2: the host program writes every edge's chi2 as the routine leaves it beside its result, and that
is what is compared with the restatement's here (relative to max(chi2, the threshold it was last compared with))."""
import copy
import os
import subprocess

import numpy as np
import pytest

import pose_inertial_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = tuple(pc.GPU_SCENES) + tuple("chain3/%d" % i for i in range(3))


def _scene(name):
    return pc.chain3()[int(name[-1])] if name.startswith("chain3") else pc.scene(name)


@pytest.fixture(scope="module")
def measured():
    return pc.measure()


def _host(tmp, flags, tag):
    exe = str(tmp / ("pose_inertial_main_" + tag))
    b = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", *flags, os.path.join(ROOT, "tests", "pose_inertial_main.cc"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    scenes = [_scene(n) for n in ALL]
    pc.write_scenes(str(tmp / "in.bin"), scenes)
    out = str(tmp / (tag + ".bin"))
    p = subprocess.run([exe, str(tmp / "in.bin"), out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-3000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    return dict(zip(ALL, pc.read_results(out, scenes)))


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    return _host(tmp_path_factory.mktemp("pose_inertial_cpu"), [], "plain")


def test_host_program_against_the_restatement(host_results):
    g, b = pc.golden(), pc.bounds()
    for name in ALL:
        sc = _scene(name)
        ref = pc.optimize(sc)
        rec, h = host_results[name]
        d = pc.differences(ref, h, sc)
        print(name, pc.decisions(h)[1:], " ".join(f"{q} {d[q] / g['D'][q]:.3f}" for q in d))
        assert "chi2" in d and (d["chi2"] > 0 or int(sc["problem"]["n"]) == 0)    # the edges' chi2 is compared, and is another computation
        assert pc.decisions(h) == pc.decisions(ref), name
        assert pc.within(d, b), (name, d, b)
        assert int(rec["n_initial"]) == int(sc["problem"]["n"])
        assert np.array_equal(rec["Rwb_f"], rec["est"]["Rwb"].astype(np.float32))      # what SetImuPoseVelocity receives
        assert np.array_equal(rec["twb_f"], rec["est"]["twb"].astype(np.float32)) and np.array_equal(rec["v_f"], rec["est"]["v"].astype(np.float32))


def test_host_program_under_the_sanitizers(tmp_path_factory, host_results):
    san = _host(tmp_path_factory.mktemp("pose_inertial_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"], "san")
    for name in ALL:
        assert pc.decisions(san[name][1]) == pc.decisions(host_results[name][1]), name
        assert pc.within(pc.differences(host_results[name][1], san[name][1], _scene(name)), pc.bounds()), name


def test_the_golden_file_is_current(measured):
    g = pc.golden()
    assert g["margin"] == pc.MARGIN and [tuple(v) for v in g["variants"]] == list(pc.VARIANTS) and tuple(g["scenes"]) == ALL
    print(measured)
    for q in pc.QUANTITIES:
        assert 0 < measured["D"][q] <= g["D"][q], q
    assert measured["chi2_margin"] >= g["chi2_margin"]


def test_flags_equal_is_a_fair_demand(measured):
    """no compared chi2 within 100 times the chi2 spread of its threshold in any variant, no singular value between 1e-7 and 1e-5,
    every variant with the same flags, counts and round lengths in every scene"""
    assert measured["variants_agree"]
    assert measured["chi2_margin"] > 100 * measured["D"]["chi2"], (measured["chi2_margin"], measured["D"]["chi2"])
    assert measured["singular_value_factor"] > 10 and measured["eigenvalue_factor"] > 10


def test_what_the_scenes_were_built_to_show():
    ref = pc.reference
    # the break rule counts every edge: N + 3 against the last KeyFrame, N + 4 against the last frame
    assert ref("n5/0")["iterations"] == [10, -1, -1, -1] and ref("n5/1")["iterations"] == [10, -1, -1, -1]
    assert ref("n6/0")["iterations"] == [10, -1, -1, -1] and ref("n6/1")["iterations"] == [10, 10, 10, 10]
    assert ref("n7/0")["iterations"] == [10, 10, 10, 10] and ref("n0/0")["iterations"] == [10, -1, -1, -1]
    for f in (0, 1):
        # the recovery arm clears flags and recounts; rec_init leaves the classification's
        a, b = ref("n29_recover/%d" % f), ref("n29_recover_recinit/%d" % f)
        assert a["n_inliers"] < 30 and a["n_inliers"] == b["n_inliers"]
        assert np.array_equal(b["flags"], b["levels"][-1]) and (a["flags"] <= a["levels"][-1]).all()
        assert b["n_bad"] == int(b["levels"][-1].sum()) and len(a["chi2"]) == 5 and len(b["chi2"]) == 4
        # the mono 1.5 x arm: a close point between t and 1.5 t stays an inlier
        r, sc = ref("close_points/%d" % f), pc.scene("close_points/%d" % f)
        c, t = r["chi2"][3]
        assert ((sc["close"] == 1) & (c > np.float32(5.991)) & (c <= t) & ~r["levels"][3]).sum() >= 3
        assert ((sc["close"] == 0) & (c > np.float32(5.991)) & r["levels"][3]).sum() >= 1
        # negative depth is an outlier whatever its chi2
        r = ref("behind_camera/%d" % f)
        assert r["flags"][-6:].all()
        # the round thresholds: out after round one, in at the end
        r = ref("outliers_40pct/%d" % f)
        assert (r["levels"][0] & ~r["flags"]).sum() >= 1
        # stale chi2: the flags come out differently if an inlier's chi2 is taken at the returned estimate
        sc = pc.scene("stale_chi2/%d" % f)
        assert (pc.optimize(sc)["flags"] != pc.optimize(sc, stale=False)["flags"]).sum() >= 1
        assert (ref("all_mono/%d" % f)["chi2"][0][1] == np.float32((12.0, 5.991)[f])).any()
    assert ref("huber_prior/1")["prior_chi2"][0] > 25.0                               # beyond delta 5
    assert ref("solver_fails/0")["solve_failed"] == [1, 1, 1, 1] and ref("solver_fails/0")["iterations"] == [1, 1, 1, 1]
    # thresholds differ by form: the same mono chi2 between 5.991 and 12 is an outlier of round one in one form only
    assert pc.CHI2_MONO[0][0] == 12.0 and pc.CHI2_MONO[1][0] == 5.991
    sizes = {int(pc.scene(n)["problem"]["n"]) for n in pc.GPU_SCENES}
    assert {0, 5, 6, 7, 29, 255, 256, 257, pc.CAPACITY, pc.CAPACITY + 1} <= sizes


def _states(sc):
    p = sc["problem"]
    F, O = pc._vertices(p["frame"]), pc._vertices(p["other"])
    Rcb, tcb = p["Rcb"].reshape(3, 3), p["tcb"]
    pc._camera(F, Rcb, tcb)
    pc._camera(O, Rcb, tcb)
    return F, O, Rcb, tcb


def _moved(st, col, step, Rcb, tcb):
    new = copy.deepcopy(st)
    u = np.zeros(15)
    u[col] = step
    pc._update(new, u, Rcb, tcb, False, "svd")
    return new


@pytest.mark.parametrize("seed", range(4))
def test_analytic_jacobians_against_central_differences(seed):
    sc = pc.build(300 + seed, 12, 1, start=8.0, mono_frac=0.5)
    F, O, Rcb, tcb = _states(sc)
    rng = np.random.default_rng(seed)
    O["bg"] = O["bg"] + rng.normal(0, 3e-3, 3)
    O["ba"] = O["ba"] + rng.normal(0, 3e-2, 3)
    # EdgeInertial.  The error reaches the other end's biases through GetDelta* in float32: dR, dV, dP move in steps of q, so a central
    # difference over 2h is off by up to 2 * (3 roundings) * q / (2h) per entry, and the rotation through LogSO3 by as much again
    # (DESIGN.md section 19).
    e, J = pc.inertial_edge(sc, F, O, False, "svd")
    pre = sc["problem"]["pre"]
    q = float(max(np.spacing(np.abs(pre[k]).astype(np.float32)).max() for k in ("dR", "dV", "dP")))
    h_bias = 1e-3
    tol_bias = 2 * 3 * q / h_bias
    assert 1e-5 < tol_bias < 5e-3
    for col in range(24):
        bias = 9 <= col < 15
        h = h_bias if bias else 1e-5
        at = lambda s: pc.inertial_edge(sc, _moved(F, col - 15, s, Rcb, tcb) if col >= 15 else F,        # noqa: E731
                                        _moved(O, col, s, Rcb, tcb) if col < 15 else O, False, "svd", jac=False)[0]
        num = (at(h) - at(-h)) / (2 * h)
        tol = tol_bias if bias else 1e-6 * max(1.0, np.abs(J[:, col]).max())
        print("inertial", col, float(np.abs(num - J[:, col]).max()), tol)
        assert np.abs(num - J[:, col]).max() <= tol, col
    assert np.abs(J[:, 9:15]).max() > 50 * tol_bias
    # EdgePriorPoseImu: double throughout
    e, J = pc.prior_edge(sc, O, False)
    for col in range(15):
        at = lambda s: pc.prior_edge(sc, _moved(O, col, s, Rcb, tcb), False, jac=False)[0]              # noqa: E731
        num = (at(1e-5) - at(-1e-5)) / 2e-5
        assert np.abs(num - J[:, col]).max() <= 1e-6 * max(1.0, np.abs(J[:, col]).max()), col
    # both visual edges: pixels, so relative to the column's size
    e, Xc, _ = pc.visual_errors(sc, F)
    J = pc.visual_jacobians(sc, Xc)
    assert (sc["ur"] >= 0).any() and (sc["ur"] < 0).any()
    for col in range(6):
        at = lambda s: pc.visual_errors(sc, _moved(F, col, s, Rcb, tcb))[0]                            # noqa: E731
        num = (at(1e-6) - at(-1e-6)) / 2e-6
        assert np.abs(num - J[:, :, col]).max() <= 1e-5 * max(1.0, np.abs(J[:, :, col]).max()), col


@pytest.mark.parametrize("form", (0, 1))
def test_a_noise_free_scene_returns_the_generators_state(form):
    """the starting values are off by 4e-3 rad, 1e-2 m and 2e-2 m/s; what float32 pixels, points and preintegration leave is below
    a tenth of that"""
    sc = pc.build(400 + form, 150, form, noise_px=0.0, imu_noise=0.0)
    r, t = pc.optimize(sc), sc["truth"]
    dR = r["est"]["Rwb"].T @ t["Rwb"]
    angle = float(np.arccos(min(1.0, (np.trace(dR) - 1) / 2)))
    print(angle, np.abs(r["est"]["twb"] - t["twb"]).max(), np.abs(r["est"]["v"] - t["v"]).max())
    assert r["n_bad"] == 0
    assert angle < 4e-4 and np.abs(r["est"]["twb"] - t["twb"]).max() < 1e-3 and np.abs(r["est"]["v"] - t["v"]).max() < 2e-3


@pytest.mark.parametrize("post", ("lapack", "jacobi"))
def test_marginalize_is_the_schur_complement(post):
    rng = np.random.default_rng(5)
    A = rng.normal(0, 1, (40, 30))
    H = A.T @ A + 0.1 * np.eye(30)
    M, s = pc.marginalize(H, post)
    want = H[15:, 15:] - H[15:, :15] @ np.linalg.solve(H[:15, :15], H[:15, 15:])
    assert np.abs(M - want).max() < 1e-11 * np.abs(want).max() and (s > 1e-6).all()
    # a direction of the marginalised block below the threshold is dropped, not inverted
    H2 = H.copy()
    v = rng.normal(0, 1, 15)
    v /= np.linalg.norm(v)
    P = np.eye(15) - np.outer(v, v)
    H2[:15, :15] = P @ H[:15, :15] @ P + 1e-9 * np.outer(v, v)
    M2, s2 = pc.marginalize(H2, post)
    assert np.isfinite(M2).all() and s2.min() < 1e-6 and np.abs(M2).max() < 10 * np.abs(H).max()
    Hc, w = pc.constraint_information(M, post)
    assert np.abs(Hc - (M + M.T) / 2).max() < 1e-10 * np.abs(M).max() and (w > 1e-12).all()
