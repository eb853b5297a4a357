"""tests/inertial_opt_cases.py, the numpy restatement of Optimizer::InertialOptimization: its own invariants, the committed
sensitivity file, the analytic Jacobians of the restated edge against central differences of its error, the generator's truth
recovered on noise-free scenes, and the three solvers on random arrowhead systems.  No GPU, no library."""
import math

import numpy as np
import pytest

import inertial_opt_cases as ic

SMALL = ("k2_mono", "k5_mono", "k9_mono", "two_chains", "lonely_keyframe", "no_edges_first", "no_edges_third", "third_huber_arm")


def test_scene_invariants():
    for name in ic.GPU_SCENES:
        sc = ic.scene(name)
        K, E = len(sc["kfs"]), len(sc["edges"])
        assert K <= 600
        R = sc["kfs"]["Rwb"].reshape(-1, 3, 3)
        assert np.abs(R @ ic.tr(R) - np.eye(3)).max() < 1e-12
        if E:
            dR = sc["edges"]["dR"].reshape(-1, 3, 3).astype(np.float64)
            assert np.abs(dR @ ic.tr(dR) - np.eye(3)).max() < 1e-6
            info = sc["info"]
            assert np.abs(info - ic.tr(info)).max() <= 1e-9 * np.abs(info).max()      # the recomposition is not exactly symmetric
            assert (np.linalg.eigvalsh((info + ic.tr(info)) / 2) > -1e-6 * np.abs(info).max()).all()
        rows, ep, en = ic.chains(sc)
        assert len(set(rows)) == len(rows) and (ep >= 0).sum() == E and (en >= 0).sum() == E


def test_the_scene_list_covers_what_the_kernel_can_get_wrong():
    sizes = {len(ic.scene(n)["kfs"]) for n in ic.GPU_SCENES}
    assert {2, 3, 5, 8, 9, 33, 257, 300, 600} <= sizes
    g = ic.golden()["scenes"]
    assert any(g[n]["rejected_trials"] > 0 for n in ic.GPU_SCENES)
    assert len(ic.chains(ic.scene("two_chains"))[0]) == 20 and (ic.chains(ic.scene("two_chains"))[1] < 0).sum() == 2
    assert (ic.chains(ic.scene("three_chains"))[1] < 0).sum() == 3
    assert len(ic.chains(ic.scene("lonely_keyframe"))[0]) == 11 and len(ic.chains(ic.scene("lonely_in_the_middle"))[0]) == 13
    # the third overload's Huber(1): every edge on the quadratic arm, exactly the outlier on the linear one, and a mix of both
    def arms(name):
        sc = ic.scene(name)
        _, at_start = ic.total_chi2(sc, ic.initial_state(sc), ic.VARIANTS[0])
        return at_start > 1.0, ic.reference(name)["chi2"] > 1.0
    start, end = arms("third")
    assert not start.any() and not end.any()
    start, end = arms("third_huber_arm")
    assert list(np.flatnonzero(start)) == [7] and list(np.flatnonzero(end)) == [7]
    for name in ("third_mixed", "third_k300"):
        start, end = arms(name)
        assert 0 < start.sum() < len(start) and not end.any(), name
    assert ic.reference("no_edges_third")["status"] == 1 and ic.reference("no_edges_first")["status"] == 0
    # the rotation JRg dbg of the large_dbg scene is far above float32's resolution of dR
    sc = ic.scene("large_dbg")
    assert np.abs(sc["edges"]["JRg"].reshape(-1, 3, 3) @ ic.reference("large_dbg")["bg"]).max() > 1e-3


@pytest.mark.parametrize("name", [n for n in ic.GPU_SCENES if len(ic.scene(n)["kfs"]) <= 33])
def test_no_decision_of_a_scene_is_left_to_rounding(name):
    trace = []
    r = ic.optimize(ic.scene(name), trace=trace)
    assert ic.counts(r) == ic.counts(ic.reference(name))
    assert ic.decision_margin(trace) >= ic.NOISY, name


def test_the_golden_file_is_current():
    g = ic.golden()
    assert g["margin"] == ic.MARGIN and [tuple(v) for v in g["variants"]] == list(ic.VARIANTS)
    assert set(g["scenes"]) == set(ic.GPU_SCENES)
    for name in ic.GPU_SCENES:
        assert g["scenes"][name]["digest"] == ic.digest(ic.scene(name)), name
        assert g["scenes"][name]["status_agrees"], name
        for q in ic.QUANTITIES:
            assert g["scenes"][name]["spread"][q] <= g["D"][q]
    agree = sum(g["scenes"][n]["counts_agree"] for n in ic.GPU_SCENES)
    assert 4 * agree >= 3 * len(ic.GPU_SCENES), agree
    again = ic.measure(SMALL)                                   # the small scenes measured again: the same numbers
    for name in SMALL:
        assert again["scenes"][name] == g["scenes"][name], name


def _numeric_jacobian(sc, st, col, h):
    """central differences of the restated error through the vertices' oplus"""
    def at(step):
        x = np.zeros(15)
        x[col] = step
        new = dict(v=st["v"].copy(), bg=st["bg"] + x[3:6], ba=st["ba"] + x[6:9], scale=st["scale"] * math.exp(x[14]),
                   Rwg=ic.mm(st["Rwg"], ic.exp_so3(x[12], x[13], 0.0)))
        new["v"][sc["edges"]["kf_prev"]] += x[0:3]                # (one edge per scene here)
        new["v"][sc["edges"]["kf_cur"]] += x[9:12]
        return ic.edge_errors(sc, new)[0]
    return (at(h) - at(-h)) / (2 * h)


@pytest.mark.parametrize("seed", range(6))
def test_analytic_jacobians_against_central_differences(seed):
    sc = ic.make_scene(seed=200 + seed, K=2, mono=True, noise=1.0)
    rng = np.random.default_rng(seed)
    t = sc["truth"]
    st = dict(v=t["v"] + rng.normal(0, 0.05, t["v"].shape), bg=t["bg"] + rng.normal(0, 3e-3, 3), ba=t["ba"] + rng.normal(0, 3e-2, 3),
              Rwg=t["Rwg"] @ ic._rot(rng.normal(0, 0.1, 3)), scale=t["scale"] * 1.1)
    err, T = ic.edge_errors(sc, st)
    J = ic.edge_jacobians(sc, st, err, T)[0]
    J[:, 14] *= st["scale"]                                       # the reference's column is d e / d s; oplus is s exp(u)
    # The error reaches the biases through GetDelta* in float32: dR, dV, dP move in steps of q (measured below), so a central
    # difference over 2h is off by up to 2 * (3 roundings) * q / (2h) per entry, and the rotation through LogSO3 by as much again.
    dR, dV, dP, _ = ic.bias_corrected(sc, st["bg"], st["ba"], False, "svd")
    q = float(max(np.spacing(np.abs(a).astype(np.float32)).max() for a in (dR, dV, dP)))
    h_bias = 1e-3
    tol_bias = 2 * 3 * q / h_bias
    assert 1e-5 < tol_bias < 5e-3
    for col in range(15):
        bias = 3 <= col < 9
        num = _numeric_jacobian(sc, st, col, h_bias if bias else 1e-5)[0]
        tol = tol_bias if bias else 1e-7 * max(1.0, np.abs(J[:, col]).max())   # double throughout: h^2 and eps / h are both 1e-10
        print(col, float(np.abs(num - J[:, col]).max()), tol)
        assert np.abs(num - J[:, col]).max() <= tol, col
    assert np.abs(J[:, 3:9]).max() > 50 * tol_bias                # the bound can tell a wrong sign


@pytest.mark.parametrize("mono", (False, True))
def test_the_first_overload_recovers_the_truth_without_noise(mono):
    sc = ic.make_scene(seed=101, K=40, mono=mono, priors=(0.0, 0.0), noise=0.0, scale_true=1.15 if mono else None)
    r, t = ic.optimize(sc), sc["truth"]
    angle = math.degrees(math.acos(min(1.0, float(t["Rwg"][:, 2] @ r["Rwg"][:, 2]))))
    print(angle, r["scale"], t["scale"], r["bg"], t["bg"], r["ba"], t["ba"])
    assert angle < 1.0
    assert abs(r["scale"] / t["scale"] - 1) < 0.01
    assert np.linalg.norm(r["bg"] - t["bg"]) < 0.1 * np.linalg.norm(t["bg"])
    assert np.linalg.norm(r["ba"] - t["ba"]) < 0.1 * np.linalg.norm(t["ba"])
    assert np.abs(r["v"] - t["v"]).max() < 0.01 * t["speed"]


@pytest.mark.parametrize("n,m", ((1, 3), (2, 9), (3, 0), (7, 9), (8, 2), (9, 6), (33, 9)))
def test_the_three_solvers_agree_on_arrowhead_systems(n, m):
    rng = np.random.default_rng(n * 16 + m)
    N = 3 * n + m
    A = rng.normal(0, 1, (N + 4, N))
    H = A.T @ A
    for r in range(n):                                            # keep the block-tridiagonal part and the border
        for c in range(n):
            if abs(r - c) > 1:
                H[3 * r:3 * r + 3, 3 * c:3 * c + 3] = 0
    H += N * np.eye(N)
    b = rng.normal(0, 1, N)
    L = dict(n=n, m=m, D=np.array([H[3 * r:3 * r + 3, 3 * r:3 * r + 3] for r in range(n)]),
             U=np.array([H[3 * r:3 * r + 3, 3 * r + 3:3 * r + 6] if r + 1 < n else np.zeros((3, 3)) for r in range(n)]),
             B=np.array([H[3 * r:3 * r + 3, 3 * n:] for r in range(n)]).reshape(n, 3, m), bv=b[:3 * n].reshape(n, 3), C=H[3 * n:, 3 * n:],
             bc=b[3 * n:])
    want = np.linalg.solve(H + 0.5 * np.eye(N), b)
    for solver in ("chain", "cyclic", "lapack"):
        xv, xb = ic.solve(L, 0.5, solver)
        assert np.abs(np.concatenate([xv.reshape(-1), xb]) - want).max() < 1e-12, solver
    L["D"][n // 2] = -L["D"][n // 2]                             # a pivot that is not positive: every solver reports it
    for solver in ("chain", "cyclic", "lapack"):
        assert ic.solve(L, 0.0, solver) is None, solver
