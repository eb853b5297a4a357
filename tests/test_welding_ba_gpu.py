"""The welding bundle adjustment of a visual map merge on the device (msorb_welding_ba, csrc/bundle_adjustment.hip) through the C
ABI against the float64 restatement of tests/welding_ba_cases.py ('forward' = g2o's order).

Bounds.  D is the largest difference between any two of the restatement's four variants over these very scenes, committed in
tests/golden/welding_ba_sensitivity.json and re-checked by tests/test_welding_ba_cpu.py.  The device adds in one more order, so its
double estimates may differ from the restatement's by 16 D, the project's rule.  The status, every count of both rounds, both
flag arrays and the active counts must be EQUAL: test_welding_ba_cpu.py shows that the four variants agree on them on every scene.
The four costs: 1e-9 relative, the cap against a wrong cost (the variants stay inside it, test_welding_ba_cpu.py).

The scenes of wc.STOP_SCENES raise the stop flag at a chosen poll through msorb_debug_welding_ba_poll_hook, which the engine calls
before every read of the flag: status 3, a round that ends on a rejected trial (stale_chi2: the flags differ from a classification
at the accepted state), a stop inside round 2, and a round 2 that makes no iteration.

A vertex that round 2's graph does not hold (kf_dropped, one_active_kf, point_dropped, all_flagged) must return what round 1 left
bit for bit.  Round 1 is not observable through the entry on its own, so the test builds it from the entry: msorb_bundle_adjustment
with 5 robust iterations runs the same engine with the same Huber widths over the same graph, and its doubles are round 1's.

Measured on an MI355X (largest |device - forward| per scene, printed by the test): 0.83 D on the points (kf_dropped; k9 and
no_edge_point 0.35 D), 0.03 D on the poses (rejected); the costs within 2.2e-10; every count and flag equal."""
import json

import numpy as np
import pytest

import local_ba_cases as lc
import welding_ba_cases as wc

pytestmark = pytest.mark.gpu

ROUND = ("iterations", "trials", "rejected_trials")


@pytest.fixture(scope="module")
def golden():
    with open(wc.GOLDEN) as f:
        return json.load(f)


def _run(msorb_mod, s, stop=None, **kw):
    """stop: a name of wc.STOPS: the library's poll hook raises the flag at that poll, every time"""
    if stop is not None:
        flag, rises = np.zeros(1, np.int32), wc.STOPS[stop]

        def hook(rnd, where, it, trials):
            if rises(rnd, where, it, trials):
                flag[0] = 1
        kw.update(stop_flag=flag, poll_hook=hook)
    return msorb_mod.welding_ba(s["kf"], s["pos_w"], s["edge_kf"], s["edge_point"], s["xy"], s["u_right"], s["inv_sigma2"], **kw)


def _same(a, b):
    return (all(a[k].tobytes() == b[k].tobytes() for k in ("kf_qt", "kf_qt_d", "pos", "pos_d", "level1", "outlier"))
            and a["result"].tobytes() == b["result"].tobytes())


def _counts(res):
    return (int(res["status"]), tuple(tuple(int(res["round"][i][k]) for k in ROUND) for i in range(2)), int(res["n_level1"]),
            int(res["n_outliers"]), int(res["active_keyframes"]), int(res["active_points"]))


def _costs(res):
    return [float(res["round"][i][k]) for i in range(2) for k in ("chi2_initial", "chi2_final")]


def test_capacity(msorb_mod):
    assert msorb_mod.welding_ba_capacity() == msorb_mod.bundle_adjustment_capacity()


@pytest.mark.parametrize("name", list(wc.ALL_SCENES))
def test_against_the_restatement(msorb_mod, golden, name):
    s, ref = wc.scene(name), wc.reference(name)
    r = _run(msorb_mod, s, stop=wc.STOP_SCENES[name][1] if name in wc.STOP_SCENES else None)
    res = r["result"]
    D, bound = golden["D"], golden["bound"]
    assert bound == 16 * D
    d_pose, d_point = lc.estimate_distance(s, dict(kf_qt_d=r["kf_qt_d"], pos_d=r["pos_d"]), ref)
    d_cost = max(wc.cost_distance(x, y) for x, y in zip(_costs(res), wc.costs(ref)))
    print(f"{name}: pose {d_pose:.3e} = {d_pose / D:.3f} D, points {d_point:.3e} = {d_point / D:.3f} D, bound {bound:.3e}; cost {d_cost:.2e}; "
          f"counts {_counts(res)} ref {wc.counts(ref)} level1_differ={int(np.sum(r['level1'] != ref['level1']))} "
          f"flags_differ={int(np.sum(r['outlier'] != ref['outlier']))} costs {_costs(res)} lambda {[float(res['round'][i]['lambda_final']) for i in range(2)]} "
          f"ref {[ref['round'][i]['lambda_final'] for i in range(2)]}")
    # the status, the counts of both rounds, both flag arrays, the active counts: equal
    assert _counts(res) == wc.counts(ref)
    assert np.array_equal(r["level1"], ref["level1"]) and np.array_equal(r["outlier"], ref["outlier"])
    assert res["n_level1"] == r["level1"].sum() and res["n_outliers"] == r["outlier"].sum()
    # the double estimates and the costs
    assert d_pose <= bound and d_point <= bound
    assert d_cost <= 1e-9
    # the float outputs: the narrowing of the device's own doubles
    assert np.array_equal(r["kf_qt"], r["kf_qt_d"].astype(np.float32)) and np.array_equal(r["pos"], r["pos_d"].astype(np.float32))
    assert np.isfinite(r["kf_qt_d"]).all() and np.isfinite(r["pos_d"]).all()
    # fixed KeyFrames: bit-equal to the input
    fixed = np.asarray(s["kf"]["fixed"]).astype(bool)
    qt_in = np.concatenate([s["kf"]["q"], s["kf"]["t"]], 1)
    assert fixed.any() and r["kf_qt"][fixed].tobytes() == qt_in[fixed].tobytes()
    assert r["kf_qt_d"][fixed].tobytes() == qt_in[fixed].astype(np.float64).tobytes()


def _round1(msorb_mod, s, n_iterations=5):
    """round 1 on the device: the engine's optimize(5) with Huber kernels of the same widths over the same graph"""
    return msorb_mod.bundle_adjustment(s["kf"], s["pos_w"], s["edge_kf"], s["edge_point"], s["xy"], s["u_right"], s["inv_sigma2"],
                                       n_iterations=n_iterations, robust=True)


@pytest.mark.parametrize("name, accepted_iterations", [("stop_between", 5), ("stop_round1", 2), ("stale_chi2", 2)])
def test_a_flag_that_is_up_after_round_1(msorb_mod, name, accepted_iterations):
    """status 3: round 1's counts, no level, no round 2, the flags of the one classification, and the estimates of round 1 bit for
    bit (the engine's own optimize(n) over the same graph; stale_chi2: its third iteration ends on the rejected trial, so the
    estimate is the one two iterations left)"""
    s, ref = wc.scene(name), wc.reference(name)
    r, one = _run(msorb_mod, s, stop=wc.STOP_SCENES[name][1]), _round1(msorb_mod, s, accepted_iterations)
    res = r["result"]
    assert res["status"] == 3 and _counts(res) == wc.counts(ref) and not r["level1"].any() and res["n_level1"] == 0
    assert [int(res["round"][1][k]) for k in ROUND] == [0, 0, 0] and res["active_keyframes"] == 0 and res["active_points"] == 0
    assert ref["round"][0]["iterations"] == accepted_iterations + (name == "stale_chi2")
    assert np.array_equal(r["outlier"], ref["outlier"]) and r["outlier"].any() and not r["outlier"].all()
    for key in ("kf_qt_d", "kf_qt", "pos_d", "pos"):
        assert r[key].tobytes() == one[key].tobytes(), key
    if name == "stop_between":          # the one classification is the one that would have made the levels
        assert np.array_equal(r["outlier"], _run(msorb_mod, s)["level1"])


def test_round_1_ends_on_a_rejected_trial_and_the_stale_chi2_decides(msorb_mod):
    """chi2 is read at the copy of the state the rejected trial wrote, the depth at the accepted one: the flags equal the
    restatement's and differ from what a classification at the accepted state gives (a kernel that reads `cur` fails here)"""
    s, ref, wrong = wc.scene("stale_chi2"), wc.reference("stale_chi2"), wc.reference("stale_chi2", chi2_at="accepted")
    r = _run(msorb_mod, s, stop="round1_rejected")
    assert ref["round"][0]["rejected_trials"] == 1 and (ref["outlier"] != wrong["outlier"]).sum() >= 10
    assert np.array_equal(r["outlier"], ref["outlier"]) and not np.array_equal(r["outlier"], wrong["outlier"])
    assert ref["kf_qt_d"].tobytes() == wrong["kf_qt_d"].tobytes()       # the estimates do not depend on it


def test_the_hook_is_gone_after_the_call(msorb_mod):
    s = wc.scene("mixed")
    _run(msorb_mod, s, stop="between")
    flag = np.zeros(1, np.int32)
    assert _same(_run(msorb_mod, s, stop_flag=flag), _run(msorb_mod, s)) and flag[0] == 0


@pytest.mark.parametrize("name", list(wc.DROPPED_KF) + list(wc.DROPPED_POINT) + ["all_flagged"])
def test_a_vertex_outside_round_2_keeps_the_bits_of_round_1(msorb_mod, name):
    s, ref = wc.scene(name), wc.reference(name)
    r, one = _run(msorb_mod, s), _round1(msorb_mod, s)
    assert [int(one["result"][k]) for k in ROUND] == [int(r["result"]["round"][0][k]) for k in ROUND]
    free = ~np.asarray(s["kf"]["fixed"]).astype(bool)
    kf_out, pt_out = free & ~ref["kf_active"], ~ref["pt_active"]
    if name in wc.DROPPED_KF:
        assert kf_out[wc.DROPPED_KF[name]] and kf_out.sum() == 1
    if name in wc.DROPPED_POINT:
        assert pt_out[wc.DROPPED_POINT[name]]
    if name == "all_flagged":
        assert kf_out.sum() == free.sum() and pt_out.all() and np.array_equal(r["level1"], r["outlier"]) and r["level1"].all()
        assert r["result"]["round"][1]["iterations"] == 0
    assert kf_out.any() or pt_out.any()
    for key, out in (("kf_qt_d", kf_out), ("kf_qt", kf_out), ("pos_d", pt_out), ("pos", pt_out)):
        assert r[key][out].tobytes() == one[key][out].tobytes(), key
    # and it did move in round 1, and what stayed in the graph moved on in round 2
    qt_in = np.concatenate([s["kf"]["q"], s["kf"]["t"]], 1)
    if kf_out.any():
        assert not np.array_equal(r["kf_qt"][kf_out], qt_in[kf_out])
    kf_in = free & ref["kf_active"]
    if kf_in.any():
        assert not np.array_equal(r["kf_qt_d"][kf_in], one["kf_qt_d"][kf_in])
    # the restatement's round 1, narrowed, within a float ulp of it
    assert np.allclose(r["kf_qt"][kf_out], ref["round1_kf_qt_d"][kf_out].astype(np.float32), rtol=2e-7, atol=1e-7)
    assert np.allclose(r["pos"][pt_out], ref["round1_pos_d"][pt_out].astype(np.float32), rtol=2e-7, atol=1e-7)


def test_a_point_without_an_edge_returns_its_input_bits(msorb_mod):
    s = wc.scene("no_edge_point")
    r = _run(msorb_mod, s)
    assert not (np.asarray(s["edge_point"]) == len(s["pos_w"]) - 1).any()
    assert r["pos"][-1].tobytes() == s["pos_w"][-1].tobytes() and r["pos_d"][-1].tobytes() == s["pos_w"][-1].astype(np.float64).tobytes()


def test_the_depth_alone_puts_an_edge_on_level_1(msorb_mod):
    s, ref = wc.scene("depth_only"), wc.reference("depth_only")
    by_depth = ~ref["chi2_flag1"] & ~(ref["depth1"] > 0)
    assert by_depth.sum() == 1
    r = _run(msorb_mod, s)
    assert r["level1"][by_depth].all() and r["outlier"][by_depth].all() and r["level1"].sum() == 1


@pytest.mark.parametrize("name", ["mixed", "k9", "rejected", "kf_dropped", "stale_chi2", "stop_round2"])
def test_two_calls_return_the_same_bits(msorb_mod, name):
    s = wc.scene(name)
    stop = wc.STOP_SCENES[name][1] if name in wc.STOP_SCENES else None
    assert _same(_run(msorb_mod, s, stop=stop), _run(msorb_mod, s, stop=stop))


def test_a_stop_flag_that_is_already_set(msorb_mod):
    s, ref = wc.scene("mixed"), wc.reference("mixed", stop="before")
    r = _run(msorb_mod, s, stop_flag=np.ones(1, np.int32))
    assert _counts(r["result"]) == wc.counts(ref) and r["result"]["status"] == 2
    assert r["kf_qt"].tobytes() == np.concatenate([s["kf"]["q"], s["kf"]["t"]], 1).tobytes()
    assert r["kf_qt_d"].tobytes() == ref["kf_qt_d"].tobytes() and r["pos_d"].tobytes() == ref["pos_d"].tobytes()
    assert r["pos"].tobytes() == s["pos_w"].tobytes() and not r["outlier"].any() and not r["level1"].any()
    assert _costs(r["result"]) == [0.0] * 4


def test_a_live_stop_flag_that_stays_clear_changes_nothing(msorb_mod):
    s = wc.scene("mixed")
    assert _same(_run(msorb_mod, s, stop_flag=np.zeros(1, np.int32)), _run(msorb_mod, s))


def test_more_free_keyframes_than_the_capacity(msorb_mod):
    cap = msorb_mod.welding_ba_capacity()
    s = wc.scene("mixed")
    kf = np.zeros(cap + 2, lc.KF_DTYPE)
    kf[:] = s["kf"][0]
    kf["fixed"] = 0
    kf["fixed"][-1] = 1
    lib = msorb_mod._wba_lib()
    E, P, K = len(s["edge_kf"]), len(s["pos_w"]), len(kf)
    qt, qtd = np.full((K, 7), 7.0, np.float32), np.full((K, 7), 7.0)
    po, pod = np.full((P, 3), 7.0, np.float32), np.full((P, 3), 7.0)
    lvl, out = np.full(E, 7, np.uint8), np.full(E, 7, np.uint8)
    res = np.full(1, 7, np.uint8).repeat(msorb_mod.WELDING_BA_RESULT_DTYPE.itemsize)
    ptr = msorb_mod._np_ptr
    xy = np.ascontiguousarray(s["xy"], np.float32)
    rc = lib.msorb_welding_ba(0, K, ptr(kf), P, ptr(s["pos_w"]), E, ptr(s["edge_kf"]), ptr(s["edge_point"]), ptr(xy), ptr(s["u_right"]),
                              ptr(s["inv_sigma2"]), None, ptr(qt), ptr(qtd), ptr(po), ptr(pod), ptr(lvl), ptr(out), ptr(res), None)
    assert rc == msorb_mod.E_CAPACITY
    for a in (qt, qtd, po, pod, lvl, out, res):       # nothing written
        assert (a == 7).all()
    with pytest.raises(msorb_mod.MsorbError) as e:
        msorb_mod.welding_ba(kf, s["pos_w"], s["edge_kf"], s["edge_point"], s["xy"], s["u_right"], s["inv_sigma2"])
    assert e.value.code == msorb_mod.E_CAPACITY


def test_edges_that_are_not_point_major_or_out_of_range(msorb_mod):
    s = wc.scene("mixed")
    for ek, ep in ((s["edge_kf"], s["edge_point"][::-1]), (s["edge_kf"] + len(s["kf"]), s["edge_point"]),
                   (s["edge_kf"], s["edge_point"] + len(s["pos_w"]))):
        with pytest.raises(msorb_mod.MsorbError) as e:
            msorb_mod.welding_ba(s["kf"], s["pos_w"], ek, ep, s["xy"], s["u_right"], s["inv_sigma2"])
        assert e.value.code == msorb_mod.E_ARG
