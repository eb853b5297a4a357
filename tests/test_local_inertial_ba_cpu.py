"""tests/local_inertial_ba_cases.py, the numpy restatement of Optimizer::LocalInertialBA, and
ms-slam_amd/csrc/local_inertial_ba_device.h compiled for the host (tests/local_inertial_ba_main.cc, once more under AddressSanitizer
and UBSan): the host program against the forward restatement, the committed sensitivity file measured again, the conditions that
make "flags and counts are equal" a fair demand, what each scene was built to show, the analytic Jacobians of the restated edges
against central differences, the generator's state recovered on a noise-free scene, and the Schur path against a dense solve of the
full system.  No GPU, no library.

Bounds.  D is, per quantity (the entries of Rwb, twb and the points over the median depth, the velocity over the speed, bg, ba,
every visual edge's chi2 as the classification reads it relative to max(chi2, threshold), the two costs relative to themselves),
the largest difference between the forward restatement and any of its variants over the scenes:
tests/golden/local_inertial_ba_sensitivity.json.  Another statement of the same arithmetic may differ from the restatement by 16 D
(DESIGN.md sections 9 to 24); status, iterations, trials, rejected trials, the flags and their count are equal.

The two arms no scene reaches (720 gross starts were tried: none ended its call on a rejected trial whose flags differ from those
at the estimate, and none met the FAIL rule in both statements) are tested on their own in the host program: --fail-rule with
hand-set err / err_end, a NaN among them, and --stale on a hand-made pair of states.  Exact zero residuals cannot be asked of
float32 observations, so no scene ends on rho == 0 either: --terminate drives lm::levenberg, the loop the engine runs, with
hand-made costs through both Terminate arms (rho == 0 after one trial, ten rejected trials) and the fork's three-bad-iterations
stop."""
import os
import subprocess

import numpy as np
import pytest

import local_inertial_ba_cases as lc
import pose_inertial_cases as pic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = tuple(lc.GPU_SCENES)


@pytest.fixture(scope="module")
def measured():
    return lc.measure()


def _build(tmp, flags, tag):
    exe = str(tmp / ("local_inertial_ba_main_" + tag))
    b = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", *flags, os.path.join(ROOT, "tests", "local_inertial_ba_main.cc"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def _host(tmp, flags, tag):
    exe = _build(tmp, flags, tag)
    scenes = [lc.scene(n) for n in ALL]
    lc.write_scenes(str(tmp / "in.bin"), scenes)
    out = str(tmp / (tag + ".bin"))
    p = subprocess.run([exe, str(tmp / "in.bin"), out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-3000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    for mode in ("--fail-rule", "--stale", "--terminate"):
        q = subprocess.run([exe, mode], capture_output=True, text=True, timeout=60)
        assert q.returncode == 0 and "runtime error" not in q.stderr, (mode, q.stdout, q.stderr[-2000:])
    return dict(zip(ALL, lc.read_results(out, scenes)))


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    return _host(tmp_path_factory.mktemp("local_inertial_ba_cpu"), [], "plain")


def test_host_program_against_the_restatement(host_results):
    g, b = lc.golden(), lc.bounds()
    for name in ALL:
        sc, ref = lc.scene(name), lc.reference(name)
        rec, ko, h = host_results[name]
        d = lc.differences(ref, h, sc)
        print(name, lc.decisions(h)[:5], " ".join(f"{q} {d[q] / g['D'][q]:.3f}" for q in d))
        assert lc.decisions(h) == lc.decisions(ref), name
        assert lc.within(d, b), (name, d, b)
        assert len(sc["edge_kf"]) == 0 or d["chi2"] > 0                        # the edges' chi2 is compared, and is another computation
        free = sc["kf"]["kind"] == 0
        for k in ("Rcw", "tcw", "v"):                                          # what the setters receive
            assert np.array_equal(ko[k + "_f"], ko[k].astype(np.float32)), (name, k)
        assert np.array_equal(ko["bias_f"], np.concatenate([ko["ba"], ko["bg"]], 1).astype(np.float32)), name
        assert np.array_equal(ko["Rwb"][~free], sc["kf"]["Rwb"][~free]) and np.array_equal(ko["tcw"][~free], sc["kf"]["tcw"][~free])


def test_host_program_under_the_sanitizers(tmp_path_factory, host_results):
    san = _host(tmp_path_factory.mktemp("local_inertial_ba_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"], "san")
    for name in ALL:
        assert lc.decisions(san[name][2]) == lc.decisions(host_results[name][2]), name
        assert lc.within(lc.differences(host_results[name][2], san[name][2], lc.scene(name)), lc.bounds()), name


def test_the_golden_file_is_current(measured):
    g = lc.golden()
    assert g["margin"] == lc.MARGIN and [tuple(v) for v in g["variants"]] == list(lc.VARIANTS) and tuple(sorted(g["scenes"])) == tuple(sorted(ALL))
    for q in lc.QUANTITIES:                                                    # the committed D is what --measure gives: never below it
        assert measured["D"][q] <= g["D"][q] and g["D"][q] <= 2 * measured["D"][q] + 1e-18, (q, measured["D"][q], g["D"][q])
    for name in ALL:
        assert measured["scenes"][name]["decisions"] == g["scenes"][name]["decisions"], name


def test_the_scenes_make_equal_decisions_a_fair_demand(measured):
    g = lc.golden()
    assert measured["variants_agree"] and g["variants_agree"]
    b = lc.bounds()
    for name in ALL:
        s = g["scenes"][name]
        # no compared chi2 within 100 times the scene's own chi2 spread of its threshold
        assert s["chi2_margin"] >= 100 * s["D"].get("chi2", 0.0), (name, s["chi2_margin"], s["D"])
        # no accept / reject decision of Levenberg within 100 times the scene's own spread of the cost
        assert s["decision_margin"] >= 100 * s["D"].get("cost", 0.0), (name, s["decision_margin"], s["D"])
        # every free vertex of every type moves further than the bound of its quantity.  The one structural exception is
        # at_optimum, which by its definition starts where it ends: nothing there may move.
        if name != "at_optimum":
            for q, moved in s["movement"].items():
                assert moved > b[q], (name, q, moved, b[q])


def test_each_scene_is_what_it_is_named_for():
    def sc(n):
        return lc.scene(n)

    def ref(n):
        return lc.reference(n)
    kinds = lambda n: sc(n)["kf"]["kind"]  # noqa: E731
    assert (kinds("n1") == 0).sum() == 1 and len(sc("n1")["ie"]) == 1 and sc("n1")["ie"][0]["huber"] == 1 and sc("n1")["ie"][0]["downweight"] == 1
    for n, k in (("n2", 2), ("n3", 3), ("n4", 4), ("n10", 10), ("n25_large", 25)):
        assert (kinds(n) == 0).sum() == k and list(sc(n)["ie"]["downweight"]) == [1] + [0] * (k - 1), n
    assert lc.CAPACITY == 25 and sc("n25_large")["large"] == 1 and ref("n25_large")["iterations"] == 4 and sc("n10")["iterations"] == 0
    # the every-third-update normalisation: three accepted updates; n4: the counter across rejected trials
    assert ref("n3")["iterations"] - 0 >= 3 and ref("n3")["rejected_trials"] == 0
    r4 = ref("n4")
    assert r4["rejected_trials"] >= 1 and r4["trials"] - r4["rejected_trials"] >= 4
    assert ref("rejected_trials")["rejected_trials"] >= 1
    s = sc("no_prev")
    first = int(np.flatnonzero(s["kf"]["kind"] == 1)[0])
    assert (s["edge_kf"] == first).sum() > 0 and list(s["ie"]["downweight"]) == [1, 0, 0] and list(s["ie"]["huber"]) == [1, 0, 0]
    assert int(s["ie"][0]["pre"]["kf_prev"]) == first
    assert sc("rec_init")["ie"]["huber"].all() and list(sc("rec_init")["ie"]["downweight"]) == [1, 0, 0]
    assert (sc("mono_only")["ur"] < 0).all() and (sc("stereo_only")["ur"] >= 0).all()
    m = sc("mixed")["ur"] < 0
    assert m.any() and (~m).any()
    s, r = sc("close_points"), ref("close_points")
    close = s["close"].astype(bool)[s["edge_pt"]]
    between = (r["chi2"] > float(lc.CHI2_MONO)) & (r["chi2"] < float(lc.CHI2_CLOSE))
    assert (between & close & ~r["flags"]).any() and (between & ~close & r["flags"]).any()
    s, r = sc("behind"), ref("behind")
    depth = lc.visual_errors(s, r["st"], r["pts"])[1][:, 2]                      # a mono point with negative depth at the end
    assert ((depth < 0) & (s["ur"] < 0)).any() and r["flags"][depth < 0].all() and ((s["ur"] >= 0) | (depth > 0) | r["flags"]).all()
    counts = lambda n: np.bincount(sc(n)["edge_pt"], minlength=len(sc(n)["pos"]))  # noqa: E731
    assert (counts("single_obs") == 1).sum() >= 3
    s = sc("fixed_only_point")
    free_edge = s["kf"]["kind"][s["edge_kf"]] == 0
    only_fixed = np.setdiff1d(np.unique(s["edge_pt"]), np.unique(s["edge_pt"][free_edge]))
    assert len(only_fixed) >= 1
    assert len(sc("p65")["pos"]) == 65 and len(sc("p257")["pos"]) == 257 and len(sc("e1025")["edge_kf"]) == 1025
    s, r = sc("outliers"), ref("outliers")
    assert s["planted"].sum() >= 20 and r["flags"][s["planted"]].mean() > 0.9
    assert ref("it1")["iterations"] == 1 and ref("it3")["iterations"] == 3
    s, r = sc("at_optimum"), ref("at_optimum")
    assert r["chi2_initial"] < 100.0 and r["rejected_trials"] == 0                             # next to nothing to gain, nothing moves
    mv = lc.movement(s, r)
    assert max(mv["twb"], mv["points"], mv["Rwb"]) < 1e-5, mv
    s = sc("realistic")
    assert (s["kf"]["kind"] == 0).sum() == 10 and (s["kf"]["kind"] != 0).sum() == 6 and len(s["pos"]) == 600
    for n in ALL:
        assert ref(n)["status"] == 0, n


def test_visual_jacobians_against_central_differences():
    sc = lc.scene("mixed")
    st, pts = lc.initial_state(sc)
    e0, Xc, _ = lc.visual_errors(sc, st, pts)
    Ja, Jb = lc.visual_jacobians(sc, st, Xc)
    h = 1e-6
    for a in range(3):                                                         # the point
        d = np.zeros(3)
        d[a] = h
        ep, _, _ = lc.visual_errors(sc, st, pts + d)
        em, _, _ = lc.visual_errors(sc, st, pts - d)
        num = (ep - em) / (2 * h)
        assert np.allclose(num, Ja[:, :, a], rtol=1e-5, atol=1e-4 * np.abs(Ja).max()), a
    free = np.flatnonzero(sc["kf"]["kind"] == 0)
    for a in range(6):                                                         # the pose: every free KeyFrame moved at once
        out = []
        for sgn in (1, -1):
            new = [dict(s) for s in st]
            u = np.zeros(15)
            u[a] = sgn * h
            for k in free:
                pic._update(new[k], u, sc["kf"][k]["Rcb"].reshape(3, 3), sc["kf"][k]["tcb"], False, "svd")
            out.append(lc.visual_errors(sc, new, pts)[0])
        num = (out[0] - out[1]) / (2 * h)
        on = np.isin(sc["edge_kf"], free)
        assert np.allclose(num[on], Jb[on, :, a], rtol=1e-4, atol=1e-4 * np.abs(Jb[on]).max()), a
        assert np.abs(num[~on]).max() == 0


def test_inertial_jacobian_against_central_differences():
    sc = lc.scene("n3")
    st, _ = lc.initial_state(sc)
    E = sc["ie"][1]
    a, b = int(E["pre"]["kf_prev"]), int(E["pre"]["kf_cur"])
    prob = dict(problem=dict(pre=E["pre"]))
    _, J = pic.inertial_edge(prob, st[b], st[a], False, "svd")
    Rcb, tcb = sc["kf"][0]["Rcb"].reshape(3, 3), sc["kf"][0]["tcb"]

    def err(which, col, step):
        O, F = dict(st[a]), dict(st[b])
        u = np.zeros(15)
        u[col] = step
        pic._update(O if which == 0 else F, u, Rcb, tcb, False, "svd")
        return pic.inertial_edge(prob, F, O, False, "svd", jac=False)[0]
    for which, cols, base in ((0, range(15), 0), (1, range(9), 15)):
        for c in cols:
            bias = which == 0 and c >= 9                                       # the bias goes through the float32 correction
            h = 1e-3 if bias else 1e-6
            num = (err(which, c, h) - err(which, c, -h)) / (2 * h)
            tol = (2e-2 if bias else 1e-5) * max(np.abs(J[:, base + c]).max(), 1.0)
            assert np.abs(num - J[:, base + c]).max() <= tol, (which, c, num, J[:, base + c])


def test_a_noise_free_scene_returns_the_generator_state():
    sc = lc.build(777, 3, 40, noise_px=0.0, imu_noise=0.0, start=3.0, point_noise=0.02)
    r = lc.optimize(sc)
    st0, pts0 = lc.initial_state(sc)
    free = np.flatnonzero(sc["kf"]["kind"] == 0)
    for k in free:
        t = sc["truth"][k]
        before = np.abs(st0[k]["twb"] - t["twb"]).max()
        after = np.abs(r["st"][k]["twb"] - t["twb"]).max()
        assert after < 1e-4 and after < before / 20, (k, before, after)
        assert np.abs(r["st"][k]["Rwb"] - t["Rwb"]).max() < 1e-4
    seen = np.bincount(sc["edge_pt"], minlength=len(pts0)) >= 2
    assert (np.abs(r["pts"] - sc["true_points"])[seen].max(axis=1) / np.linalg.norm(sc["true_points"][seen], axis=1)).max() < 1e-3
    assert r["chi2_final"] < 1e-3 * r["chi2_initial"] and r["n_outliers"] == 0


def test_the_schur_path_equals_a_dense_solve_of_the_full_system():
    sc = lc.scene("n2")
    var = lc.VARIANTS[0]
    st, pts = lc.initial_state(sc)
    L = lc.linearise(sc, st, pts, var)
    lam = 1.0
    x, xl, solved = lc.solve_trial(sc, L, lam, var, None)
    assert solved
    free, free_of, idx = lc.unknowns(sc)
    n, P = 15 * len(free), len(pts)
    H = np.zeros((n + 3 * P, n + 3 * P))
    H[:n, :n] = np.triu(L["H"]) + np.triu(L["H"], 1).T
    for e in range(len(sc["edge_kf"])):
        i, p = free_of[sc["edge_kf"][e]], sc["edge_pt"][e]
        if i >= 0:
            H[6 * i:6 * i + 6, n + 3 * p:n + 3 * p + 3] += L["W"][e]
    H[n:, :n] = H[:n, n:].T
    for p in range(P):
        Hl = np.triu(L["Hll"][p]) + np.triu(L["Hll"][p], 1).T
        H[n + 3 * p:n + 3 * p + 3, n + 3 * p:n + 3 * p + 3] = Hl
    H += lam * np.eye(n + 3 * P)
    full = np.linalg.solve(H, np.concatenate([L["b"], L["bl"].reshape(-1)]))
    a = lc.apply_update(sc, st, pts, x, xl, var)
    b = lc.apply_update(sc, st, pts, full[:n], full[n:].reshape(-1, 3), var)
    D = lc.golden()["D"]
    ra = dict(st=a[0], pts=a[1], chi2=np.zeros(0), thr=np.zeros(0), chi2_final=1.0, chi2_initial=1.0)
    rb = dict(st=b[0], pts=b[1], chi2=np.zeros(0), thr=np.zeros(0), chi2_final=1.0, chi2_initial=1.0)
    d = lc.differences(ra, rb, sc)
    assert all(d[k] <= D[k] for k in ("Rwb", "twb", "v", "bg", "ba", "points")), (d, D)
    assert np.abs(x).max() > 1e-4
