"""The float64 restatement of the welding bundle adjustment (tests/welding_ba_cases.py) on its own, and the conditions its named
scenes must meet for tests/test_welding_ba_gpu.py to mean something.  No GPU.

D (the unit of the GPU test's bound, 16 D) is the largest difference between any two of the restatement's variants over the
scenes: tests/golden/welding_ba_sensitivity.json, regenerated here."""
import json

import numpy as np
import pytest

import local_ba_cases as lc
import welding_ba_cases as wc


@pytest.fixture(scope="module")
def golden():
    with open(wc.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def measured():
    return wc.measure()


def test_the_committed_golden_is_what_measure_gives(golden, measured):
    """sin / cos come from the platform's libm, so the re-measured figures may move in their last bits: within a factor of two"""
    print(json.dumps({k: measured[k] for k in ("D", "bound", "cost")}), "committed", {k: golden[k] for k in ("D", "bound", "cost")})
    assert set(golden["scenes"]) == set(wc.ALL_SCENES) == set(measured["scenes"])
    assert golden["bound"] == 16 * golden["D"]
    assert golden["D"] / 2 <= measured["D"] <= 2 * golden["D"] and golden["cost"] / 2 <= measured["cost"] <= 2 * golden["cost"]
    assert 0 < golden["D"] < 1e-8
    # scene by scene: the flags that say "agree" equal, D and the cost within the same factor (a figure at rounding level, below
    # 1e-12, may move by more than that between two libms: there both must be below 1e-12)
    for name, g in golden["scenes"].items():
        m = measured["scenes"][name]
        assert (g["counts_agree"], g["flags_agree"]) == (m["counts_agree"], m["flags_agree"]), name
        for k in ("D", "cost"):
            assert g[k] / 2 <= m[k] <= 2 * g[k] or max(g[k], m[k]) < 1e-12, (name, k, g[k], m[k])


def test_the_variants_agree_on_every_flag_and_count(measured):
    """what the GPU test demands to be EQUAL is equal between the four variants, on every scene"""
    for name, v in measured["scenes"].items():
        assert v["flags_agree"] and v["counts_agree"], (name, [wc.counts(wc.reference(name, x)) for x in wc.VARIANTS])


def test_the_variants_stay_inside_the_cap_on_the_costs(measured):
    """the GPU test's 1e-9 on the four costs: no two variants are further apart than half of it on any scene, so a fifth order of
    summation that strays as far from `forward` as the other three do still has as much room again"""
    for name, v in measured["scenes"].items():
        assert v["cost"] <= 5e-10, (name, v["cost"])


def test_both_rounds_run_and_the_second_graph_is_smaller():
    r = wc.reference("mixed")
    s = wc.scene("mixed")
    assert r["status"] == 0 and r["round"][0]["iterations"] == 5 and r["round"][1]["iterations"] > 0
    assert 0 < r["n_level1"] < len(r["level1"]) and r["active_points"] < len(s["pos_w"])
    st = np.asarray(s["u_right"]) >= 0
    assert st.any() and (~st).any() and r["level1"][st].any() and r["level1"][~st].any()
    assert s["planted"].sum() >= 0.1 * len(st)
    assert r["round"][1]["chi2_initial"] < r["round"][0]["chi2_final"]        # the flagged edges took their cost with them


def test_a_clean_scene_flags_nothing():
    r = wc.reference("clean")
    assert r["n_level1"] == 0 and r["n_outliers"] == 0 and r["active_points"] == len(wc.scene("clean")["pos_w"])
    assert r["round"][1]["iterations"] > 0


def test_mono_only_and_stereo_only():
    assert not (np.asarray(wc.scene("mono_only")["u_right"]) >= 0).any()
    assert (np.asarray(wc.scene("stereo_only")["u_right"]) >= 0).all()
    for name in ("mono_only", "stereo_only"):
        assert 0 < wc.reference(name)["n_level1"] < len(wc.reference(name)["level1"])


@pytest.mark.parametrize("name", list(wc.DROPPED_KF))
@pytest.mark.parametrize("variant", wc.VARIANTS)
def test_a_free_keyframe_without_an_active_edge_keeps_round_1(name, variant):
    s, r = wc.scene(name), wc.reference(name, variant)
    k = wc.DROPPED_KF[name]
    mine = np.asarray(s["edge_kf"]) == k
    assert 3 <= mine.sum() <= 4 and r["level1"][mine].all() and not r["kf_active"][k] and not s["kf"]["fixed"][k]
    assert r["kf_qt_d"][k].tobytes() == r["round1_kf_qt_d"][k].tobytes()
    others = r["kf_active"]
    assert others.sum() == r["active_keyframes"] == (1 if name == "one_active_kf" else 2)
    assert not np.array_equal(r["kf_qt_d"][others], r["round1_kf_qt_d"][others])
    q0 = np.asarray(s["kf"]["q"][k], np.float64)
    assert np.abs(r["kf_qt_d"][k, :4] - q0 / np.linalg.norm(q0)).max() > 1e-6       # round 1 did move it


@pytest.mark.parametrize("variant", wc.VARIANTS)
def test_a_point_without_an_active_edge_keeps_round_1(variant):
    s, r = wc.scene("point_dropped"), wc.reference("point_dropped", variant)
    p = wc.DROPPED_POINT["point_dropped"]
    mine = np.asarray(s["edge_point"]) == p
    assert mine.sum() >= 2 and r["level1"][mine].all() and not r["pt_active"][p]
    assert r["pos_d"][p].tobytes() == r["round1_pos_d"][p].tobytes()
    assert not np.array_equal(r["pos_d"][r["pt_active"]], r["round1_pos_d"][r["pt_active"]])


def test_every_edge_flagged_leaves_round_2_nothing():
    r = wc.reference("all_flagged")
    assert r["level1"].all() and r["round"][1] == dict(iterations=0, trials=0, rejected_trials=0, chi2_initial=0.0, chi2_final=0.0, lambda_final=0.0)
    assert np.array_equal(r["outlier"], r["level1"]) and r["active_keyframes"] == 0 and r["active_points"] == 0
    assert r["kf_qt_d"].tobytes() == np.where(np.asarray(wc.scene("all_flagged")["kf"]["fixed"]).astype(bool)[:, None], r["kf_qt_d"], r["round1_kf_qt_d"]).tobytes()
    assert r["round"][0]["rejected_trials"] > 0


def test_round_1_rejects_trials():
    r = wc.reference("rejected")
    assert r["round"][0]["rejected_trials"] > 0 and r["round"][0]["trials"] == 5 + r["round"][0]["rejected_trials"]


def test_the_depth_alone_flags_an_edge():
    """the point behind the last fixed KeyFrame: chi2 far under the threshold at the trial state, the depth negative"""
    s, r = wc.scene("depth_only"), wc.reference("depth_only")
    by_depth = ~r["chi2_flag1"] & ~(r["depth1"] > 0)
    assert by_depth.sum() == 1 and by_depth[-1] and r["chi2_trial1"][-1] < 1.0
    assert r["level1"][-1] and r["outlier"][-1] and r["depth"][-1] < 0 and not r["chi2_flag"][-1]
    assert r["n_level1"] == 1


def test_the_classification_alone():
    """the rules of :3726-3753 and :3769-3803 on hand-made edges: the double comparison, the depth, and what a level-1 edge keeps"""
    stereo = np.array([False, False, True, True, False, False])
    # the comparison is in double: 5.991 and 7.815 themselves are not greater.  LocalBundleAdjustment narrows chi2 to float first
    # (:1339), and (float)5.991 = 5.99100018 is greater than the double 5.991: the same edge is flagged there and not here
    chi2 = np.array([5.991, np.nextafter(5.991, 6), 7.815, np.nextafter(7.815, 8), np.nan, 0.0])
    assert wc.chi2_flags(chi2, stereo).tolist() == [False, True, False, True, False, False]
    assert float(np.float32(5.991)) > 5.991
    # the depth decides alone, whatever the chi2 flag; a depth of exactly zero or NaN is "not positive"
    assert wc.classify([False, False, False, True, True], [1.0, 0.0, -1.0, 1.0, np.nan]).tolist() == [False, True, True, True, True]
    # the stale rule: a level-1 edge flagged by chi2 in round 1 stays flagged though its chi2 and depth are fine at the end;
    # one flagged by the depth alone follows the final depth
    flag1, depth1 = np.array([True, False, False]), np.array([1.0, -1.0, 1.0])
    level1 = wc.classify(flag1, depth1)
    assert level1.tolist() == [True, True, False]
    flag = flag1.copy()
    flag[~level1] = wc.chi2_flags(np.array([1.0]), np.array([False]))          # only the active edge is refreshed
    assert wc.classify(flag, np.array([1.0, 1.0, 1.0])).tolist() == [True, False, False]
    assert wc.classify(flag, np.array([1.0, -1.0, 1.0])).tolist() == [True, True, False]


def test_the_stale_chi2_of_a_level_1_edge_stays():
    """on a scene: at the final state some level-1 edge has a chi2 under its threshold and a positive depth, and is flagged still"""
    s, r = wc.scene("k9"), wc.reference("k9")
    pr = lc.Problem(s)
    q, t = r["kf_qt_d"][:, :4].copy(), r["kf_qt_d"][:, 4:].copy()
    free = ~pr.fixed
    q[~free] = np.array([wc.normalize_rotation(v) for v in q[~free]])
    _, p, chi2 = pr.error(q, t, r["pos_d"])
    fresh = wc.classify(wc.chi2_flags(chi2, pr.stereo), p[:, 2])
    stale = r["level1"] & ~fresh
    assert stale.any() and r["outlier"][stale].all()
    assert (r["outlier"] & ~r["level1"]).any()                                # and round 2 flagged an edge round 1 had kept


def test_nine_free_keyframes_are_more_than_one_panel():
    s = wc.scene("k9")
    assert 6 * int((~np.asarray(s["kf"]["fixed"]).astype(bool)).sum()) > 48 and wc.reference("k9")["active_keyframes"] == 9


def test_a_point_without_an_edge_is_a_vertex_that_does_not_move():
    s, r = wc.scene("no_edge_point"), wc.reference("no_edge_point")
    assert not (np.asarray(s["edge_point"]) == len(s["pos_w"]) - 1).any()
    assert r["pos"][-1].tobytes() == s["pos_w"][-1].tobytes()


def test_the_restated_loop_with_terminate_is_local_ba_cases_loop():
    """wc.levenberg with a flag that stays down returns the bits of lc.levenberg, on the scene with rejected trials"""
    a, b = wc.welding_ba(wc.scene("rejected"), "forward", stop=lambda *x: False), wc.reference("rejected")
    assert a["kf_qt_d"].tobytes() == b["kf_qt_d"].tobytes() and a["pos_d"].tobytes() == b["pos_d"].tobytes()
    assert wc.counts(a) == wc.counts(b) and wc.costs(a) == wc.costs(b) and np.array_equal(a["outlier"], b["outlier"])
    assert [a["round"][i]["lambda_final"] for i in range(2)] == [b["round"][i]["lambda_final"] for i in range(2)]


def test_round_1_ends_on_a_rejected_trial_and_the_stale_chi2_matters():
    """the flag rises right after round 1's first rejected trial: chi2() belongs to the discarded trial state.  A statement that
    classifies at the accepted state gives a DIFFERENT flag set, so a kernel that reads the wrong copy fails the GPU test"""
    s = wc.scene("stale_chi2")
    r, wrong, full = wc.reference("stale_chi2"), wc.reference("stale_chi2", chi2_at="accepted"), wc.reference("rejected")
    assert r["status"] == 3 and r["round"][0]["rejected_trials"] == 1 and r["round"][0]["trials"] == r["round"][0]["iterations"]
    assert r["round"][0]["iterations"] < 5 and full["round"][0]["rejected_trials"] > 1
    differ = r["outlier"] != wrong["outlier"]
    print("flags that differ", int(differ.sum()), "of", len(differ), "set", int(r["outlier"].sum()), "against", int(wrong["outlier"].sum()))
    assert differ.sum() >= 10 and r["kf_qt_d"].tobytes() == wrong["kf_qt_d"].tobytes() and not r["level1"].any()
    # the depth is the accepted state's in both
    assert np.array_equal(r["depth"], wrong["depth"])
    # and the variants agree on the flags, so equality on the device is a fair demand
    for v in wc.VARIANTS:
        assert np.array_equal(wc.reference("stale_chi2", v)["outlier"], r["outlier"]), v


def test_a_stop_inside_a_round():
    one, two, first = wc.reference("stop_round1"), wc.reference("stop_round2"), wc.reference("stop_round2_first")
    assert one["status"] == 3 and one["round"][0]["iterations"] == 2 and not one["level1"].any() and one["outlier"].any()
    assert two["status"] == 0 and two["round"][1]["iterations"] == 3 and two["level1"].any()
    assert np.array_equal(two["level1"], wc.reference("k9")["level1"])
    # round 2 without an iteration: the levels are made, and every edge keeps round 1's chi2: the final flags are the levels
    full = wc.reference("mixed")
    assert first["status"] == 0 and first["round"][1]["iterations"] == 0 and np.array_equal(first["level1"], full["level1"])
    assert np.array_equal(first["outlier"], first["level1"]) and first["active_points"] == full["active_points"]
    free = ~np.asarray(wc.scene("mixed")["kf"]["fixed"]).astype(bool)
    assert first["kf_qt_d"][free].tobytes() == first["round1_kf_qt_d"][free].tobytes() and first["pos_d"].tobytes() == first["round1_pos_d"].tobytes()


def test_the_stop_flag():
    s = wc.scene("mixed")
    r = wc.reference("mixed", stop="before")
    assert wc.counts(r) == (2, ((0, 0, 0), (0, 0, 0)), 0, 0, 0, 0)
    assert r["kf_qt"].tobytes() == np.concatenate([s["kf"]["q"], s["kf"]["t"]], 1).tobytes() and r["pos"].tobytes() == s["pos_w"].tobytes()
    b, full = wc.reference("mixed", stop="between"), wc.reference("mixed")
    assert b["status"] == 3 and b["round"][0] == full["round"][0] and b["round"][1]["iterations"] == 0
    assert not b["level1"].any() and np.array_equal(b["outlier"], full["level1"])      # the one classification is round 1's
    assert b["kf_qt_d"].tobytes() == np.where(np.asarray(s["kf"]["fixed"]).astype(bool)[:, None], b["kf_qt_d"], full["round1_kf_qt_d"]).tobytes()


def test_local_ba_for_15_iterations_is_another_routine():
    """what this feature exists for: 15 iterations of LocalBundleAdjustment's loop (Huber throughout, one graph, one classification
    at the accepted state) do not give the welding routine's estimates or flags on the outlier scene"""
    s, r = wc.scene("mixed"), wc.reference("mixed")
    other = lc.local_ba(s, "forward", 15)
    d = max(lc.estimate_distance(s, r, other))
    print("distance", d, "flags differ", int((other["outlier"] != r["outlier"]).sum()))
    assert d > 1e-6                                   # the GPU test's bound is below 1e-8
    assert (other["outlier"] != r["outlier"]).any()
