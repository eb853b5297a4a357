"""The float64 restatement of Optimizer::OptimizeSim3 (tests/sim3_opt_cases.py) on its own: it solves what it should, takes the
reference's early return, and its variants (three summation orders, a libm nudged by one ulp) bound what the kernel's tree and
the device's libm may change.  No GPU."""
import json
import math

import numpy as np

import sim3_opt_cases as sc


def test_recovers_a_noise_free_similarity_and_flags_the_planted_outliers():
    """double inputs without noise, 20 % planted outliers, free and fixed scale: exactly the planted pairs are bad and the
    estimate comes back.  How far is set by the routine, not by the arithmetic: it stops at its budget of 5 + 10 damped steps, not
    at convergence.  Measured here: 1.8e-7 (200 pairs), 2.5e-5 (60 pairs, the kept pairs' chi2 still 1.6e-6 px^2) and 9e-13 (fixed
    scale), the same for every variant.  Asserted: every kept pair reprojects within 1e-2 px in both images (chi2 < 1e-4), which at
    fx = 719 is an angle of 1.4e-5 rad, and the estimate lies within 1e-4 of the planted one."""
    for seed, n, fix in ((101, 200, False), (102, 60, False), (103, 200, True)):
        s = sc.make_scene(seed, n, outliers=0.2, noise=0.0, fix_scale=fix, dtype=np.float64)
        for variant in sc.VARIANTS:
            r = sc.run(s, sum_order=variant[0], nudge=variant[1])
            truth = dict(q=s["q_true"], t=s["t_true"], s=s["s_true"])
            d = sc.estimate_difference(r, truth, 1.0)
            print(seed, variant, d, r["iterations"], r["rejected_trials"], r["n_bad"], r["n_in"])
            assert d < 1e-4 and np.max(r["chi2"][r["bad"] == 0]) < 1e-4
            assert 0 < s["planted"].sum() < n and np.array_equal(r["bad"] == 1, s["planted"]) and not (r["bad"] == 2).any()
            assert r["status"] == 0 and r["n_bad"] == int(s["planted"].sum()) and r["n_in"] == n - r["n_bad"]
            if fix:
                assert r["s"] == 1.0


def test_early_return_below_the_minimum():
    """n - nBad < min_pairs (:2211-2212, :2397-2398): 0 is returned before g2oS12 is written, after the first optimisation ran
    and the first classification reset its matches.  n = 0: nothing runs."""
    r, s = sc.reference("n0"), sc.scene("n0")
    assert r["status"] == 1 and r["iterations"] == [-1, -1] and r["n_in"] == 0
    for name in ("n1", "n4", "n9", "all_bad"):
        r, s = sc.reference(name), sc.scene(name)
        assert r["status"] == 1 and r["n_in"] == 0 and r["iterations"][0] >= 1 and r["iterations"][1] == -1, name
        assert r["q"].tobytes() == s["q"].tobytes() and r["t"].tobytes() == s["t"].tobytes() and r["s"] == s["s"], name
        assert r["n_bad"] == int((r["bad"] == 1).sum()) and not (r["bad"] == 2).any(), name
    r = sc.reference("all_bad")
    assert r["n_bad"] == r["n_pairs"] == 40 and (r["bad"] == 1).all()          # the step-2 flags are kept
    for name in ("n5", "n10"):                                                  # exactly the minimum: the second run is made
        r = sc.reference(name)
        assert r["status"] == 0 and r["iterations"][1] >= 1 and r["n_in"] == r["n_pairs"], name


def test_the_second_run_gets_its_2_when_nothing_is_bad_and_its_1_otherwise():
    """nMoreIterations (:2205-2209).  This fork's _nBad rule usually stops a run before its budget, so the arm is shown by a
    budget of one: the run the routine takes stops after one solve, the other budget changes nothing."""
    clean, dirty = sc.scene("clean"), sc.scene("n63")
    assert sc.reference("clean")["n_bad"] == 0 and sc.reference("n256")["n_bad"] == 0 and sc.reference("n63")["n_bad"] > 0
    assert 1 < sc.reference("clean")["iterations"][1] <= 5 and 1 < sc.reference("n63")["iterations"][1] <= 10
    assert sc.run(clean, its=(5, 10, 1))["iterations"][1] == 1
    assert sc.run(clean, its=(5, 1, 5))["iterations"] == sc.reference("clean")["iterations"]
    assert sc.run(dirty, its=(5, 1, 5))["iterations"][1] == 1
    assert sc.run(dirty, its=(5, 10, 1))["iterations"] == sc.reference("n63")["iterations"]


def test_the_rejected_trials_scene_pops_trials_in_the_first_run():
    """so the stale-error rule (the first classification reads the chi2 of the last trial, popped or not) is exercised"""
    for v in sc.VARIANTS:
        assert sc.reference("rejected_trials", v)["rejected_trials"][0] > 0


def test_the_first_classification_reads_what_the_last_trial_left():
    """the chi2 the first classification reads is the last trial's.  Where that trial was accepted it is the chi2 at the estimate the
    run ended on, bit for bit.  A run ends on a POPPED trial only when ten in a row fail (levenberg.cpp:149-155); the `converged`
    scene starts at the optimum for that, and is the one scene whose first run takes that exit.  By then lambda has grown by
    2^55 and the popped step no longer moves a bit of the estimate, so the stale chi2 equals the estimate's there too: the rule
    is restated because it is the reference's, and it is printed, not asserted, whether it shows."""
    popped = accepted = 0
    for name in sc.GPU_SCENES:
        s, r = sc.scene(name), sc.reference(name)
        if r["first_run"] is None:
            continue
        E = sc.Pairs(s["cam1"], s["cam2"], s["P1c"], s["P2c"], s["obs1"], s["obs2"], s["w1"], s["w2"], s["th2"])
        S = r["first_run"]["S"]
        _, _, at_estimate = E.errors(S, sc.sim3_inverse(S))
        same = np.array_equal(r["chi2_read"][0], at_estimate, equal_nan=True)
        if r["first_run"]["last_trial_popped"]:
            popped += 1
            print(name, "ends on a popped trial; stale chi2 equals the estimate's:", same)
            assert r["rejected_trials"][0] >= 10, name
        else:
            accepted += 1
            assert same, name
    assert popped >= 1 and accepted >= 2 and sc.reference("converged")["first_run"]["last_trial_popped"], (popped, accepted)


def test_fixed_scale_zeroes_column_6_and_keeps_the_bits_of_s():
    s = sc.scene("n64")
    assert s["fix_scale"]
    log = []
    r = sc.run(s, jac_log=log)
    assert len(log) == sum(r["iterations"])
    for J12, J21 in log:
        assert not J12[:, :, 6].any() and not J21[:, :, 6].any()               # exactly 0, not small
        assert np.abs(J12[:, :, :6]).max() > 1 and np.abs(J21[:, :, :6]).max() > 1
    assert r["s"] == s["s"]
    log = []
    sc.run(sc.scene("n63"), jac_log=log)
    # free scale: the column is there for e21; e12 projects e^sigma (s R x + t), which the projection cannot see: rounding noise only
    assert np.abs(log[0][1][:, :, 6]).max() > 1 and np.abs(log[0][0][:, :, 6]).max() < 1e-2


def test_the_pair_behind_camera_2_is_behind_and_takes_part():
    s = sc.scene("behind")
    S = ([float(v) for v in s["q"]], [float(v) for v in s["t"]], s["s"])
    z = sc.sim3_map(sc.sim3_inverse(S), np.asarray(s["P1c"], np.float64))[:, 2]
    assert z[-1] < 0 and (z[:-1] > 0).all()
    r = sc.reference("behind")
    assert r["bad"][-1] == 1 and r["status"] == 0 and np.isfinite(r["q"]).all()


def test_sensitivity_matches_the_committed_golden():
    """D, C and the margin over the GPU scenes, full and one-step, as `python tests/sim3_opt_cases.py --measure` wrote them.  exp,
    sin and cos come from the platform's libm, so the re-measured figures may move: within a factor of two of the committed ones."""
    with open(sc.GOLDEN) as f:
        g = json.load(f)
    m = sc.measure()
    for tag, gg, mm in (("full", g, m), ("one_step", g["one_step"], m["one_step"])):
        print(tag, {k: mm[k] for k in ("D", "C", "margin")}, "committed", {k: gg[k] for k in ("D", "C", "margin")})
        assert set(gg["scenes"]) == set(sc.ONE_STEP if tag == "one_step" else sc.GPU_SCENES)
        assert gg["estimate_bound"] == 16 * gg["D"] and gg["chi2_bound"] == 16 * gg["C"]
        assert gg["D"] / 2 <= mm["D"] <= 2 * gg["D"]
        assert gg["C"] / 2 <= mm["C"] <= 2 * gg["C"]
        assert 0 < gg["D"] < 1e-6 and 0 < gg["C"] < 1e-4


def test_threshold_margin():
    """no chi2 that a classification of a GPU scene reads, in any variant, full or one-step, lies within 100 C of th2: the
    kernel's summation tree and libm cannot flip a flag.  A seed that fails here is replaced in sim3_opt_cases.GPU_SCENES."""
    m = sc.measure()
    for tag, mm in (("full", m), ("one_step", m["one_step"])):
        print(tag, "margin", mm["margin"], "100 C", 100 * mm["C"])
        assert math.isfinite(mm["margin"]) and mm["margin"] > 100 * mm["C"]
