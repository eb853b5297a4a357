"""Optimizer::BundleAdjustment on the device (csrc/bundle_adjustment.hip) through the C ABI against the float64 restatement of
tests/bundle_adjustment_cases.py ('forward' = g2o's order).

Bounds.  D is the largest difference between any two of the restatement's variants (three summation orders, the reduced system
through LAPACK, and up to 40 free KeyFrames the elimination without a Schur complement) over these very scenes, committed in
tests/golden/bundle_adjustment_sensitivity.json and re-checked by tests/test_bundle_adjustment_cpu.py.  The device adds in one
more order, so its double estimates may differ from the restatement's by 16 D (DESIGN sections 9, 10, 16).  The costs are held to
1e-9 relative: a cap against a wrong cost, not a measurement; the restatement's variants stay inside it (the CPU test).

Measured on an MI355X: DESIGN.md section 16."""
import json

import numpy as np
import pytest

import bundle_adjustment_cases as bc
import local_ba_cases as lc

pytestmark = pytest.mark.gpu

COUNTS = ("status", "iterations", "trials", "rejected_trials", "n_outliers")
ARGS = ("kf", "pos_w", "edge_kf", "edge_point", "xy", "u_right", "inv_sigma2")
ESTIMATES = ("kf_qt_d", "pos_d", "kf_qt", "pos")


@pytest.fixture(scope="module")
def golden():
    with open(bc.GOLDEN) as f:
        return json.load(f)


def _run(msorb_mod, s, **kw):
    kw.setdefault("n_iterations", s["n_iterations"])
    kw.setdefault("robust", s["robust"])
    if s["stop"]:
        kw.setdefault("stop_flag", np.ones(1, np.int32))
    return msorb_mod.bundle_adjustment(*(s[k] for k in ARGS), **kw)


def _same(a, b):
    return (all(a[k].tobytes() == b[k].tobytes() for k in ("kf_qt", "kf_qt_d", "pos", "pos_d", "point_included"))
            and a["result"].tobytes() == b["result"].tobytes())


@pytest.mark.parametrize("name", list(bc.SCENES))
def test_against_the_restatement(msorb_mod, golden, name):
    s, ref = bc.scene(name), bc.reference(name)
    r = _run(msorb_mod, s)
    res = r["result"]
    D, bound = golden["D"], golden["bound"]
    assert bound == 16 * D
    d_pose, d_point = lc.estimate_distance(s, dict(kf_qt_d=r["kf_qt_d"], pos_d=r["pos_d"]), ref)
    rel = [abs(res[k] - ref[k]) / abs(ref[k]) if ref[k] else abs(res[k]) for k in ("chi2_initial", "chi2_final")]
    print(f"{name}: pose {d_pose:.3e} = {d_pose / D:.4f} D, points {d_point:.3e} = {d_point / D:.4f} D, bound {bound:.3e}; "
          f"counts {[int(res[k]) for k in COUNTS]} ref {[ref[k] for k in COUNTS]} chi2 {res['chi2_initial']:.6f} -> {res['chi2_final']:.6f} "
          f"ref {ref['chi2_initial']:.6f} -> {ref['chi2_final']:.6f} relative {rel[0]:.2e} {rel[1]:.2e}")
    assert d_pose <= bound and d_point <= bound
    assert np.array_equal(r["kf_qt"], r["kf_qt_d"].astype(np.float32)) and np.array_equal(r["pos"], r["pos_d"].astype(np.float32))
    assert np.array_equal(r["point_included"], ref["point_included"])
    assert [int(res[k]) for k in COUNTS] == [ref[k] for k in COUNTS]
    assert rel[0] <= 1e-9 and rel[1] <= 1e-9
    assert np.isfinite(r["kf_qt_d"]).all() and np.isfinite(r["pos_d"]).all()
    # a fixed KeyFrame and a point that is no vertex: bit-equal to the input
    fixed = np.asarray(s["kf"]["fixed"]).astype(bool)
    assert r["kf_qt"][fixed].tobytes() == np.concatenate([s["kf"]["q"], s["kf"]["t"]], 1)[fixed].tobytes()
    assert r["pos"][~r["point_included"]].tobytes() == s["pos_w"][~r["point_included"]].tobytes()


def test_the_robust_switch(msorb_mod):
    a, b = _run(msorb_mod, bc.scene("not_robust")), _run(msorb_mod, bc.scene("not_robust_twin"))
    assert max(lc.estimate_distance(bc.scene("not_robust"), a, b)) > 1e-4
    assert a["result"]["chi2_initial"] > 2 * b["result"]["chi2_initial"]


@pytest.mark.parametrize("name", ["rejected", "k200_loop"])
def test_two_calls_return_the_same_bits(msorb_mod, name):
    s = bc.scene(name)
    assert _same(_run(msorb_mod, s), _run(msorb_mod, s))


def test_a_live_stop_flag_that_stays_clear_changes_nothing(msorb_mod):
    s = bc.scene("mono_init")
    assert _same(_run(msorb_mod, s, stop_flag=np.zeros(1, np.int32)), _run(msorb_mod, s))


def test_against_local_ba_on_a_problem_both_accept(msorb_mod, golden):
    s = bc.scene("k24_small")
    a = msorb_mod.local_ba(*(s[k] for k in ARGS), max_iterations=10)
    b = _run(msorb_mod, s, n_iterations=10, robust=True)
    ra, rb = a["result"], b["result"]
    d = lc.estimate_distance(s, a, b)
    print(f"local_ba vs bundle_adjustment: pose {d[0]:.3e}, points {d[1]:.3e}, bound {golden['bound']:.3e}")
    assert [int(ra[k]) for k in COUNTS[:4]] == [int(rb[k]) for k in COUNTS[:4]]
    assert max(d) <= golden["bound"]
    # one engine, the same kernels, stereo edges only (the mono Huber widths differ), and two solvers that return the same bits
    assert all(a[k].tobytes() == b[k].tobytes() for k in ESTIMATES)


@pytest.fixture(scope="module")
def k128():
    """local BA at its capacity: 128 free KeyFrames, n = 768 = 16 panels of the blocked solve (one panel up to n = 48; the largest
    other scene that both entries take has 24 free KeyFrames).  Stereo edges only, as k24_small; not an entry of SCENES, so no
    golden D moves.  K = 129, P = 400, E = 2378; the restatements: 5 iterations, 5 trials, none rejected, 0.45 s each."""
    s = bc._without_mono_edges(bc.make_windowed_scene(seed=39, free=128, points=400, stereo=1.0))
    return s, lc.local_ba(s, "forward", 5), bc.bundle_adjustment(s, "forward", 5, True, False)


def test_local_ba_at_its_capacity_against_this_entry(msorb_mod, golden, k128):
    s, ref_local, ref = k128
    assert int((s["kf"]["fixed"] == 0).sum()) == msorb_mod.local_ba_capacity() == 128
    a = msorb_mod.local_ba(*(s[k] for k in ARGS), max_iterations=5)
    b = msorb_mod.bundle_adjustment(*(s[k] for k in ARGS), n_iterations=5, robust=True)
    d = [lc.estimate_distance(s, r, ref) for r in (a, b)]
    print(f"k128: local_ba {d[0][0]:.3e} {d[0][1]:.3e}, bundle_adjustment {d[1][0]:.3e} {d[1][1]:.3e}, bound {golden['bound']:.3e}; "
          f"counts {[int(a['result'][k]) for k in COUNTS[:4]]} {[int(b['result'][k]) for k in COUNTS[:4]]} ref {[ref[k] for k in COUNTS[:4]]}")
    assert all(a[k].tobytes() == b[k].tobytes() for k in ESTIMATES)
    assert [int(a["result"][k]) for k in COUNTS[:4]] == [int(b["result"][k]) for k in COUNTS[:4]] == [ref[k] for k in COUNTS[:4]]
    assert max(max(x) for x in d) <= golden["bound"]
    assert np.array_equal(a["outlier"], ref_local["outlier"])


def test_the_existing_entry_refuses_the_chain_and_this_one_does_not(msorb_mod):
    s = bc.scene("k129_chain")
    with pytest.raises(msorb_mod.MsorbError) as e:
        msorb_mod.local_ba(*(s[k] for k in ARGS))
    assert e.value.code == msorb_mod.E_CAPACITY
    assert _run(msorb_mod, s)["result"]["iterations"] == 5


def test_more_free_keyframes_than_the_capacity(msorb_mod):
    cap = msorb_mod.bundle_adjustment_capacity()
    K = cap + 1
    kf = np.zeros(K, lc.KF_DTYPE)
    kf[:] = bc.scene("mono_init")["kf"][1]
    kf["fixed"] = 0
    L = msorb_mod._gba_lib()
    pw = np.tile(np.float32([0, 0, 10]), (K, 1))
    ek = ep = np.arange(K, dtype=np.int32)                 # one edge per KeyFrame, point-major
    xy, ur, inv = np.full((K, 2), 300, np.float32), np.full(K, -1, np.float32), np.ones(K, np.float32)
    qt, qtd = np.full((K, 7), 7, np.float32), np.full((K, 7), 7, np.float64)
    po, pod, inc = np.full((K, 3), 7, np.float32), np.full((K, 3), 7, np.float64), np.full(K, 7, np.uint8)
    res = np.full(1, 7, np.int32).repeat(12).view(msorb_mod.BA_RESULT_DTYPE)
    before = [a.copy() for a in (qt, qtd, po, pod, inc, res)]
    p = msorb_mod._np_ptr
    rc = L.msorb_bundle_adjustment(0, K, p(kf), K, p(pw), K, p(ek), p(ep), p(xy), p(ur), p(inv), 5, 1, None, p(qt), p(qtd), p(po),
                                   p(pod), p(inc), p(res), None)
    assert rc == msorb_mod.E_CAPACITY
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, (qt, qtd, po, pod, inc, res)))
