"""The float64 restatement of Optimizer::PoseOptimization (tests/pose_opt_cases.py) on its own: it solves what it should, and the
three summation orders bound what a fourth (the kernel's tree) may change.  No GPU."""
import json
import math

import numpy as np

import pose_opt_cases as pc


def test_recovers_a_noise_free_pose_and_flags_the_planted_outliers():
    """double inputs, mono edges (the stereo projection narrows 1/z to float, types_six_dof_expmap.cpp:340): the pose comes back to
    1e-9 and exactly the planted observations are outliers"""
    for seed, n in ((101, 400), (102, 60)):
        s = pc.make_scene(seed, n, stereo=0.0, outliers=0.15, noise=0.0, rot_deg=2.0, trans=0.2, dtype=np.float64)
        for order in pc.ORDERS:
            r = pc.pose_optimization(s["cam"], s["q"], s["t"], s["xy"], s["u_right"], s["inv_sigma2"], s["pos_w"], order)
            dq = np.max(np.abs(pc.sign_aligned(r["qd"], s["q_true"]) - s["q_true"]))
            dt = np.max(np.abs(r["td"] - s["t_true"]))
            print(seed, order, dq, dt, r["iterations"], r["rejected_trials"])
            assert dq < 1e-9 and dt < 1e-9
            assert 0 < s["planted"].sum() < n and np.array_equal(r["outlier"], s["planted"])
            assert r["n_initial"] == n and r["n_bad"] == int(s["planted"].sum())


def test_early_exits():
    """< 3 edges: 0 returned, nothing touched (:936-937); < 10 edges: one round (:1026-1027); an empty active set: no solve"""
    r = pc.reference("n2")
    s = pc.scene("n2")
    assert r["n_initial"] - r["n_bad"] == 0 and not r["outlier"].any() and np.array_equal(r["q"], s["q"]) and np.array_equal(r["t"], s["t"])
    assert pc.reference("n9")["iterations"][1:] == [-1, -1, -1] and pc.reference("n9")["iterations"][0] > 0
    assert min(pc.reference("n10")["iterations"]) > 0
    r = pc.reference("all_outliers")
    assert r["n_bad"] == r["n_initial"] and r["iterations"][0] > 0 and r["iterations"][1:] == [0, 0, 0]


def test_the_rejected_trials_scene_rejects_trials():
    """so the stale-error rule (the chi2 of a popped trial is what the classification reads) is exercised by the GPU tests"""
    assert sum(pc.reference("rejected_trials")["rejected_trials"]) > 0


def test_the_point_behind_the_camera_is_behind_and_finite():
    s = pc.scene("behind")
    E = pc.Edges(s["cam"], s["xy"], s["u_right"], s["inv_sigma2"], s["pos_w"])
    _, p, chi2 = E.error(pc.normalize_rotation(s["q"].astype(np.float64)), s["t"].astype(np.float64))
    assert p[-1, 2] < 0 and np.isfinite(chi2).all()
    assert np.isfinite(pc.reference("behind")["qd"]).all()


def test_order_sensitivity_matches_the_committed_golden():
    """D (pose) and C (per-edge chi2) over the GPU scenes, as `python tests/pose_opt_cases.py --measure` wrote them.  sin / cos come
    from the platform's libm, so the re-measured figures may move in their last bits: within a factor of two of the committed ones."""
    with open(pc.GOLDEN) as f:
        g = json.load(f)
    m = pc.measure()
    print(json.dumps({k: m[k] for k in ("D", "C", "pose_bound", "margin")}), "committed", {k: g[k] for k in ("D", "C", "pose_bound", "margin")})
    assert set(g["scenes"]) == set(pc.GPU_SCENES)
    assert g["pose_bound"] == 16 * g["D"]
    assert g["D"] / 2 <= m["D"] <= 2 * g["D"]
    assert g["C"] / 2 <= m["C"] <= 2 * g["C"]
    assert 0 < g["D"] < 1e-12      # a few ulps of a unit quaternion's components: the optimisation converges, it does not drift


def test_threshold_margin():
    """no chi2 of any GPU scene, round or order lies within 1e-6 (relative) of its threshold, and 1e-6 >= 100 C: a fourth summation
    order cannot flip a classification.  A seed that fails here is replaced in pose_opt_cases.GPU_SCENES."""
    worst = math.inf
    for name in pc.GPU_SCENES:
        th = pc.thresholds(pc.scene(name))
        for order in pc.ORDERS:
            for rnd, chi2 in enumerate(pc.reference(name, order)["chi2"]):
                if len(chi2) == 0:
                    continue
                rel = np.abs(chi2 - th) / th
                assert np.isfinite(rel).all(), (name, order, rnd)
                assert rel.min() > 1e-6, (name, order, rnd, rel.min())
                worst = min(worst, float(rel.min()))
    C = pc.measure()["C"]
    print("smallest margin", worst, "C", C)
    assert 1e-6 >= 100 * C
