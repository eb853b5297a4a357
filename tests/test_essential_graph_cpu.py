"""The float64 restatement of Optimizer::OptimizeEssentialGraph (tests/essential_graph_cases.py) against what the reference's rules
imply, and the committed sensitivity record against the scenes.  No GPU, no library."""
import numpy as np
import pytest

import essential_graph_cases as ec


def test_the_golden_record_matches_the_scenes():
    g = ec.golden()
    assert set(g["scenes"]) == set(ec.GPU_SCENES)
    for name in ec.GPU_SCENES:
        rec = g["scenes"][name]
        assert rec["digest"] == ec.digest(ec.scene(name)), name
        assert rec["variants_agree"], name          # the condition for a GPU scene
        assert rec["iterations"] == ec.scene(name)["iterations"], name
        assert tuple(rec["counts"]) == ec.counts(ec.reference(name)), name
    assert g["D"] == max(r["spread"] for r in g["scenes"].values()) > 0
    noisy = sum(ec.reference(n)["chi2_final"] > 1e-6 for n in ec.GPU_SCENES)
    assert 2 * noisy >= len(ec.GPU_SCENES)


@pytest.mark.parametrize("free_scale", [False, True], ids=["fixed_scale", "free_scale"])
def test_a_consistent_graph_reaches_the_variants_floor(free_scale):
    """measurements from planted poses, estimates perturbed: the optimum has zero cost.  The yardsticks are the variants' own: the
    cost each of them gives the planted poses (rounding of the measurements alone) and the spread of their results.  With free
    scale the reference stalls where its second linearisation enters Sim3::log's small-angle branch with sigma != 0 (see
    essential_graph_cases.SHORT): every variant must stall at the same cost."""
    sc = ec.consistent_graph(free_scale)
    act, _, _ = ec.active_set(sc)
    rs = [ec.optimize(sc, v) for v in ec.VARIANTS]
    spread = max(ec.estimate_difference(a["estimates"], b["estimates"]) for a in rs for b in rs)
    planted = max(ec.cost_at(sc, sc["true"], act, v[0], v[1]) for v in ec.VARIANTS)
    lo, hi = min(r["chi2_final"] for r in rs), max(r["chi2_final"] for r in rs)
    for v, r in zip(ec.VARIANTS, rs):
        err = ec.estimate_difference(r["estimates"], sc["true"])
        print(v, ec.counts(r), f"chi2 {r['chi2_initial']:.3e} -> {r['chi2_final']:.3e}; cost of the planted poses {planted:.3e}; "
              f"from the planted poses {err:.3e}; variants' spread {spread:.3e}")
        assert r["chi2_initial"] > 1e-3
        if not free_scale:
            assert err <= ec.MARGIN * max(spread, float(np.sqrt(planted)))
    assert hi <= ec.MARGIN * max(lo, planted)
    assert len({ec.counts(r)[0] for r in rs}) == 1


def test_fixed_scale_leaves_the_seventh_column_zero_and_s_untouched():
    sc = ec.scene("seven_free")
    act, free_of, vof = ec.active_set(sc)
    _, H, b = ec.linearise(sc, sc["est"], act, free_of, ec.perturbation_table(False), "forward", False)
    rows = np.arange(6, len(b), 7)
    assert not H[rows].any() and not H[:, rows].any() and not b[rows].any()      # exactly zero, not merely small
    r = ec.reference("seven_free")
    assert r["iterations"] > 0 and r["solver_failures"] == 0                       # the pivots 0 + lambda pass !(d > 0)
    assert r["estimates"][:, 7].tobytes() == sc["est"][:, 7].tobytes()
    assert (r["estimates"][:, 7] == 1.0).all()
    # the merge form: only the fixed class has _fix_scale, the free vertices' scales move
    m = ec.reference("merge_classes")
    free = ec.scene("merge_classes")["fixed"] == 0
    assert (m["estimates"][free, 7] != ec.scene("merge_classes")["est"][free, 7]).all()


def test_a_both_fixed_edge_and_an_edgeless_vertex_change_nothing():
    sc = ec.scene("active_set")
    act, free_of, vof = ec.active_set(sc)
    assert (sc["v0"][5], sc["v1"][5]) == (6, 7) and 5 not in act and free_of[8] == -1 and not sc["fixed"][8]
    keep = np.array([e for e in range(len(sc["v0"])) if not (sc["fixed"][sc["v0"][e]] and sc["fixed"][sc["v1"][e]])])
    without = dict(sc, v0=sc["v0"][keep], v1=sc["v1"][keep], meas=sc["meas"][keep])
    a, b = ec.reference("active_set"), ec.optimize(without, iterations=sc["iterations"])
    assert ec.counts(a) == ec.counts(b)
    assert (a["chi2_initial"], a["chi2_final"]) == (b["chi2_initial"], b["chi2_final"])
    assert a["estimates"].tobytes() == b["estimates"].tobytes()
    assert a["estimates"][8].tobytes() == sc["est"][8].tobytes()                  # bit for bit
    fixed = sc["fixed"] != 0
    assert a["estimates"][fixed].tobytes() == sc["est"][fixed].tobytes()


def test_both_exits_are_taken():
    stops = {name: ec.reference(name)["stop"] for name in ec.GPU_SCENES}
    ten = [n for n in ec.GPU_SCENES if stops[n] == 1 and ec.reference(n)["rejected_trials"] >= 10]
    n_bad = [n for n in ec.GPU_SCENES if stops[n] == 2]
    print("ten rejected trials:", ten, "; _nBad:", n_bad)
    assert ten and n_bad
    at = ec.reference("at_optimum")
    assert ec.counts(at) == (0, 1, 10, 10, 0, 1)                                   # ten rejected trials in a row, Terminate


def test_the_log_scene_takes_every_branch():
    sc = ec.scene("log_branches")
    act, _, _ = ec.active_set(sc)
    seen = set()
    for est in (sc["est"], ec.reference("log_branches")["estimates"]):
        E = ec.sim_mul(ec.sim_mul(sc["meas"][act], est[sc["v0"][act]]), ec.sim_inv(est[sc["v1"][act]]))
        seen.update(int(v) for v in ec.log_branches(E))
        sigma = np.log(E[:, 7])
        assert (sigma == 0.0).any() and (sigma != 0.0).any()                       # sigma = 0 exactly, and not
    print("branches of Sim3::log taken by the base errors:", sorted(seen))
    assert seen == {0, 1, 2, 3}


def test_the_restated_log_inverts_the_exponential():
    rng = np.random.default_rng(5)
    for rot, sig in ((1e-3, 0.0), (0.8, 0.0), (1e-3, 0.3), (0.8, 0.3)):
        u = np.concatenate([rng.normal(0, 1, 3) * rot, rng.normal(0, 1, 3), [sig]])
        S = ec._sim_of(*ec.sim3_exp([float(v) for v in u]))
        back = ec.sim_log(S)[0]
        print(rot, sig, np.abs(back - u).max())
        if not (rot < 1e-2 and sig):   # (the reference's small-angle branch with sigma != 0 is no inverse: its B lacks a term)
            assert np.abs(back - u).max() < 1e-8
