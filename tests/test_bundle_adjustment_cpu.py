"""The float64 restatement of Optimizer::BundleAdjustment (tests/bundle_adjustment_cases.py) on its own and the conditions its
named scenes must meet for tests/test_bundle_adjustment_gpu.py to mean something.  No GPU."""
import json

import numpy as np
import pytest

import bundle_adjustment_cases as bc
import local_ba_cases as lc


@pytest.fixture(scope="module")
def golden():
    with open(bc.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def measured():
    return bc.measure()


def test_the_committed_golden_is_what_measure_gives(golden, measured):
    """D as `python tests/bundle_adjustment_cases.py --measure` wrote it.  sin / cos come from the platform's libm and the lapack
    variant from the platform's LAPACK, so the re-measured figure may move: within a factor of two of the committed one."""
    print(json.dumps({k: measured[k] for k in ("D", "chi2", "bound")}), "committed", {k: golden[k] for k in ("D", "chi2", "bound")})
    assert set(golden["scenes"]) == set(bc.SCENES)
    assert golden["bound"] == 16 * golden["D"]
    assert golden["D"] / 2 <= measured["D"] <= 2 * golden["D"]
    assert 0 < golden["D"] < 1e-6


def test_the_variants_agree_on_the_counts(measured):
    """iterations, trials and rejected trials are equal in all variants of every scene (no scene is excused)"""
    for name, v in measured["scenes"].items():
        assert v["variants_agree"], (name, [bc.counts(bc.reference(name, x)) for x in bc.variants_of(bc.scene(name))])


def test_the_cost_of_the_variants_stays_inside_the_cap_of_the_gpu_test(measured):
    """the GPU test holds chi2_initial and chi2_final to 1e-9 relative: the variants must themselves stay inside that"""
    for name, v in measured["scenes"].items():
        assert v["chi2"] < 1e-9, (name, v["chi2"])


def test_every_free_vertex_moves_further_than_the_bound(measured):
    """the free vertex that moves least goes at least 1e3 * 16 D from its input, so the bound of the GPU test tells a kernel that
    skipped a vertex from a correct one"""
    for name, v in measured["scenes"].items():
        if name != "it0_stop":
            assert v["movement"] is not None and v["movement"] >= 1e3 * 16 * measured["D"], (name, v["movement"], measured["D"])


def test_the_special_scenes_are_what_they_are_named_for():
    s = bc.scene("mono_init")
    assert s["kf"]["fixed"].tolist() == [1, 0] and len(s["pos_w"]) == 100 and not (s["u_right"] >= 0).any() and s["n_iterations"] == 20
    assert np.bincount(s["edge_point"]).tolist() == [2] * 100
    a, b = bc.scene("not_robust"), bc.scene("not_robust_twin")
    assert all(np.array_equal(a[k], b[k]) for k in ("kf", "pos_w", "edge_kf", "edge_point", "xy", "u_right", "inv_sigma2"))
    assert (a["robust"], b["robust"]) == (False, True) and (~a["kf"]["fixed"].astype(bool)).sum() == 8 and a["kf"]["fixed"].sum() == 1
    ra, rb = bc.reference("not_robust"), bc.reference("not_robust_twin")
    assert max(lc.estimate_distance(a, ra, rb)) > 1e-4 and ra["chi2_initial"] > 2 * rb["chi2_initial"]    # the switch does something
    s, r = bc.scene("no_edge_points"), bc.reference("no_edge_points")
    assert np.nonzero(~r["point_included"])[0].tolist() == list(bc.NO_EDGE_POINTS) and len(s["pos_w"]) == 40
    assert r["pos"][~r["point_included"]].tobytes() == s["pos_w"][~r["point_included"]].tobytes()
    s, r = bc.scene("it0_stop"), bc.reference("it0_stop")
    assert bc.counts(r) == (0, 0, 0, 0) and r["pos"].tobytes() == s["pos_w"].tobytes()
    assert bc.reference("rejected")["rejected_trials"] > 0
    s, r = bc.scene("k129_chain"), bc.reference("k129_chain")
    fixed = s["kf"]["fixed"].astype(bool)
    assert (~fixed).sum() == 129 and fixed.sum() == 1 and len(s["pos_w"]) == 400 and np.bincount(s["edge_point"]).tolist() == [6] * 400
    spread = [np.ptp(s["edge_kf"][s["edge_point"] == p]) for p in range(400)]
    assert max(spread) < 8 and r["iterations"] == 5
    pl = bc.Problem(s).plan
    assert len(pl.pair_key) < pl.Kf * 8                    # the reduced system has empty blocks
    s, r = bc.scene("k200_loop"), bc.reference("k200_loop")
    fixed = s["kf"]["fixed"].astype(bool)
    assert (~fixed).sum() == 200 and fixed.sum() == 1 and not s["robust"] and r["iterations"] == 10
    assert (s["u_right"] >= 0).any() and not (s["u_right"] >= 0).all() and s["planted"].any()
    loop = [p for p in range(len(s["pos_w"])) if np.ptp(s["edge_kf"][s["edge_point"] == p]) > 150]
    assert len(loop) == 40
    s = bc.scene("k24_small")
    assert (~s["kf"]["fixed"].astype(bool)).sum() == 24 and s["kf"]["fixed"].sum() == 6 and len(s["pos_w"]) == 600
    for name in bc.SCENES:                                 # point-major, as the ABI demands
        assert (np.diff(bc.scene(name)["edge_point"]) >= 0).all(), name


def test_the_dense_variant_runs_where_it_is_affordable():
    assert [n for n in bc.SCENES if "dense" not in bc.variants_of(bc.scene(n))] == ["k129_chain", "k200_loop"]
