"""The float64 restatement of Optimizer::OptimizeEssentialGraph4DoF (tests/essential_graph4_cases.py) against what the reference's
rules imply, and the committed sensitivity record against the scenes.  No GPU, no library.

The zeroing of DR(0,2), DR(1,2), DR(2,0), DR(2,1) after every fifth accepted update (G2oTypes.cc:237-245) is restated, and the
scene ten_updates passes it twice, but it cannot be told apart from its absence here: every update multiplies DR by
ExpSO3(0, 0, u), an exact rotation about z whose four entries are zero already, so they stay zero.  No check is invented for it."""
import numpy as np

import essential_graph4_cases as ec


def test_the_golden_record_matches_the_scenes_and_the_variants_agree():
    g = ec.golden()
    assert set(g["scenes"]) == set(ec.GPU_SCENES) and len(ec.GPU_SCENES) >= 14
    D = 0.0
    for name in ec.GPU_SCENES:
        rec = g["scenes"][name]
        assert rec["digest"] == ec.digest(ec.scene(name)), name
        assert rec["variants_agree"], name          # the condition for a GPU scene
        assert rec["iterations"] == ec.scene(name)["iterations"], name
        rs = [ec.reference(name, v) for v in ec.VARIANTS]
        assert {ec.counts(r) for r in rs} == {tuple(rec["counts"])}, name        # status and counts, every variant
        spread = max(ec.pose_difference(a["poses"], b["poses"]) for a in rs for b in rs)
        assert spread == rec["spread"], (name, spread, rec["spread"])
        for r in rs:
            assert ec.lambda_agrees(r["lambda_initial"], rs[0]["lambda_initial"]), name
        D = max(D, spread)
    assert g["D"] == D > 0
    print(f"D = {D:.3e}")
    noisy = sum(ec.reference(n)["chi2_final"] > 1e-6 for n in ec.GPU_SCENES)
    assert 2 * noisy >= len(ec.GPU_SCENES)


def test_the_information_is_the_references_and_weights_the_terms():
    assert ec.OMEGA.tolist() == [1e3, 1e3, 1.0, 1.0, 1.0, 1.0]                     # (0, 0) set twice, (2, 2) never
    sc = ec.scene("kf11")
    act, free_of, vof = ec.active_set(sc)
    st = ec.initial_state(sc)
    tab = ec.perturbation_table(False, "svd")
    cost, H, b = ec.linearise(sc, st, act, free_of, tab, "forward", False)
    err = ec.error_vectors(sc, st, act, tab, False)
    e = err[0]
    assert np.isclose(cost, float((e * e * ec.OMEGA).sum()), rtol=1e-13)
    # H and b against J^T Omega J and J^T Omega (-e) formed as one dense product
    n = 4 * len(vof)
    J = np.zeros((6 * len(act), n))
    for a, ed in enumerate(act):
        for side, v in ((0, sc["v0"][ed]), (1, sc["v1"][ed])):
            if free_of[v] >= 0:
                for c in range(4):
                    J[6 * a:6 * a + 6, 4 * free_of[v] + c] = ec.SCALAR * (err[1 + 8 * side + 2 * c, a] - err[2 + 8 * side + 2 * c, a])
    Om = np.tile(ec.OMEGA, len(act))
    assert np.allclose(H, J.T @ (Om[:, None] * J), rtol=1e-9, atol=1e-9 * np.abs(H).max())
    assert np.allclose(b, -J.T @ (Om * e.reshape(-1)), rtol=1e-9, atol=1e-9 * np.abs(b).max())
    assert np.array_equal(H, H.T)


def test_lambda_starts_from_the_largest_diagonal_entry():
    for name in ("kf11", "hub70", "one_sided"):
        sc, trace = ec.scene(name), []
        r = ec.optimize(sc, iterations=1, trace=trace)
        assert r["lambda_initial"] == 1e-5 * np.abs(np.diag(trace[0]["H"])).max() > 0
        assert r["lambda_initial"] == ec.reference(name)["lambda_initial"]


def test_a_both_fixed_edge_and_an_edgeless_vertex_change_nothing():
    sc = ec.scene("active_set")
    act, free_of, vof = ec.active_set(sc)
    assert (sc["v0"][5], sc["v1"][5]) == (6, 7) and 5 not in act and free_of[8] == -1 and not sc["fixed"][8]
    keep = np.array([e for e in range(len(sc["v0"])) if not (sc["fixed"][sc["v0"][e]] and sc["fixed"][sc["v1"][e]])])
    without = dict(sc, v0=sc["v0"][keep], v1=sc["v1"][keep], meas=sc["meas"][keep])
    a, b = ec.reference("active_set"), ec.optimize(without, iterations=sc["iterations"])
    assert ec.counts(a) == ec.counts(b)
    assert (a["chi2_initial"], a["chi2_final"]) == (b["chi2_initial"], b["chi2_final"])
    assert a["poses"].tobytes() == b["poses"].tobytes()
    out = free_of < 0
    assert out[8] and a["poses"][out].tobytes() == ec.input_poses(sc)[out].tobytes()   # bit for bit


def test_the_exits_the_update_count_and_the_log_branches():
    stops = {name: ec.reference(name)["stop"] for name in ec.GPU_SCENES}
    assert stops["noisy_nbad"] == 2 and ec.reference("noisy_nbad")["chi2_final"] > 1.0
    at = ec.reference("at_optimum")
    assert ec.counts(at) == (0, 1, 10, 10, 0, 1)                                   # ten rejected trials in a row, Terminate
    assert at["poses"].tobytes() == ec.input_poses(ec.scene("at_optimum")).tobytes()
    ten = ec.reference("ten_updates")
    assert ten["accepted"] >= 10 and ten["chi2_final"] < 1e-3 * ten["chi2_initial"]  # `its` reaches 5 twice

    def exits(name, st):
        sc = ec.scene(name)
        act, _, _ = ec.active_set(sc)
        v0, v1 = sc["v0"][act], sc["v1"][act]
        dR = sc["meas"][act, :9].reshape(-1, 3, 3)
        return set(int(v) for v in ec.log_exits(ec.mm(ec.mm(st["Rcw"][v0], ec.tr(st["Rcw"][v1])), ec.tr(dR))))

    early = exits("at_optimum", ec.initial_state(ec.scene("at_optimum")))
    print("LogSO3 exits at the optimum:", sorted(early))
    assert early and 2 not in early                                               # only the two early exits
    rad = ec.reference("radian")
    assert exits("radian", rad["state"]) == {2}
    sc = ec.scene("radian")
    act, _, _ = ec.active_set(sc)
    e = ec.edge_errors(rad["state"]["Rcw"][sc["v0"][act]], rad["state"]["tcw"][sc["v0"][act]], rad["state"]["Rcw"][sc["v1"][act]],
                       rad["state"]["tcw"][sc["v1"][act]], sc["meas"][act])
    assert (np.linalg.norm(e[:, :3], axis=1) > 0.8).sum() >= 2                     # residual rotations of about a radian remain


def test_both_constructors_and_a_real_tcb():
    kf, co = ec.scene("keyframe_built"), ec.scene("corrected_built")

    def gap(sc):   # how far the camera pose handed in is from the one the body pose implies
        R, t = ec.camera_pose(sc, np.arange(len(sc["fixed"])), np.tile(ec.I3, (len(sc["fixed"]), 1, 1)), sc["twb"])
        return float(max(np.abs(R - sc["Rcw"]).max(), np.abs(t - sc["tcw"]).max()))

    print("camera pose against the body pose's: KeyFrame-built", gap(kf), "corrected", gap(co))
    assert 1e-9 < gap(kf) < 1e-5 and gap(co) < 1e-5                                # a float rounding (in the second, mTcb's own)
    for k in ("Rcw", "tcw", "Rwb", "twb"):                                         # ImuCamPose(pKF): four floats, widened
        assert np.array_equal(kf[k], kf[k].astype(np.float32).astype(np.float64)), k
    assert np.array_equal(co["Rwb"], ec.mm(ec.tr(co["Rcw"]), co["Rcb"]))           # ImuCamPose(Rwc, twc, pKF): Rwb = Rwc Rcb in double
    assert not np.array_equal(co["Rwb"], co["Rwb"].astype(np.float32).astype(np.float64))
    mixed = ec.scene("kf11")                                                       # the other scenes mix the two
    isf = [np.array_equal(mixed["Rwb"][k], mixed["Rwb"][k].astype(np.float32).astype(np.float64)) for k in range(len(mixed["fixed"]))]
    assert any(isf) and not all(isf)
    assert np.abs(ec.RCB - ec.I3).max() > 0.5 and np.abs(ec.TCB).min() > 0.01
    assert np.allclose(ec.RCB @ ec.RCB.T, ec.I3, atol=1e-14)


def test_exp_and_log_restated():
    rng = np.random.default_rng(5)
    w = rng.normal(0, 1, (50, 3))
    w = w / np.linalg.norm(w, axis=1)[:, None] * np.array([1e-7, 1e-3, 0.5, 1.5, 3.0]).repeat(10)[:, None]   # angles below pi
    R = ec.exp_so3(w[:, 0], w[:, 1], w[:, 2])
    assert np.abs(ec.mm(R, ec.tr(R)) - ec.I3).max() < 1e-14
    back = ec.log_so3(R)
    assert np.abs(back - w).max() < 1e-8
    polar = ec.exp_so3(w[:, 0], w[:, 1], w[:, 2], ortho="polar")
    assert 0 <= np.abs(polar - R).max() < 1e-14                                    # the second route to U V^T
