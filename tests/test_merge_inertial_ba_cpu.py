"""tests/merge_inertial_ba_cases.py, the numpy restatement of Optimizer::MergeInertialBA, and
ms-slam_amd/csrc/merge_inertial_ba_device.h compiled for the host (tests/merge_inertial_ba_main.cc: a serial executor, the
column-by-column solve, eg::levenberg from lambda 1e3 with the stop callable; once more under AddressSanitizer and UBSan): the host
program against the forward restatement, the committed sensitivity file measured again, the conditions that make "decisions are
equal" a fair demand, and what each scene was built to show.  No GPU, no library.

Bounds.  D is, per quantity (the entries of Rwb, twb and the points over the median depth, the velocity over the speed, bg, ba, a
classified chi2 relative to the larger of itself and its threshold, the two costs relative to themselves), the largest difference
between the forward restatement and any of its variants: tests/golden/merge_inertial_ba_sensitivity.json.  An estimate is bound by
16 D.  Status, iterations, trials, rejected trials, every outlier flag and point_included are equal."""
import os
import subprocess

import numpy as np
import pytest

import merge_inertial_ba_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = mc.ALL


@pytest.fixture(scope="module")
def measured():
    return mc.measure()


def run_host(tmp, flags, tag):
    exe = str(tmp / ("merge_inertial_ba_main_" + tag))
    b = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", *flags, os.path.join(ROOT, "tests", "merge_inertial_ba_main.cc"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    scenes = [mc.scene(n) for n in ALL]
    mc.write_scenes(str(tmp / "in.bin"), scenes)
    out = str(tmp / (tag + ".bin"))
    p = subprocess.run([exe, str(tmp / "in.bin"), out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-3000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    return dict(zip(ALL, mc.read_results(out, scenes)))


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    return run_host(tmp_path_factory.mktemp("merge_inertial_ba_cpu"), [], "plain")


def check_outputs(sc, rec, ko, r):
    """what every statement of the routine owes its caller, whatever it computed"""
    kind = sc["kf"]["kind"]
    for k in ("Rcw", "tcw", "v"):                                              # what the setters receive
        assert np.array_equal(ko[k + "_f"], ko[k].astype(np.float32)), k
    assert np.array_equal(ko["bias_f"], np.concatenate([ko["ba"], ko["bg"]], 1).astype(np.float32))   # IMU::Bias's order
    fixed = (kind == 1) | (kind == 2)
    if int(rec["status"]) != 0:
        fixed = np.ones(len(kind), bool)
        assert not r["flags"].any() and not r["included"].any()
    for k in ("Rwb", "twb", "Rcw", "tcw", "v", "bg", "ba"):                    # a fixed KeyFrame repeats its input
        assert np.array_equal(ko[k][fixed], sc["kf"][k][fixed]), k
    pose_only = kind == 3
    for k in ("v", "bg", "ba"):                                                # a pose-only KeyFrame's velocity and biases come back
        assert np.array_equal(ko[k][pose_only], sc["kf"][k][pose_only]), k
    out = ~np.asarray(r["included"], bool)
    assert np.array_equal(r["pts"][out], sc["pos"].astype(np.float64)[out])    # a point that is no vertex repeats its position
    assert not r["flags"][out[sc["edge_pt"]]].any() and int(rec["n_outliers"]) == int(r["flags"].sum())


def test_host_program_against_the_restatement(host_results):
    D = mc.golden()["D"]
    for name in ALL:
        sc, ref = mc.scene(name), mc.reference(name)
        rec, ko, h = host_results[name]
        d = mc.differences(ref, h, sc)
        print(name, mc.decisions(h)[:4], int(rec["n_outliers"]), " ".join(f"{q} {d[q] / D[q]:.3f}" for q in d if D[q] > 0))
        assert mc.decisions(h) == mc.decisions(ref), name
        assert mc.within(d, mc.bounds()), (name, d, mc.bounds())
        check_outputs(sc, rec, ko, h)


def test_host_program_under_the_sanitizers(tmp_path_factory, host_results):
    san = run_host(tmp_path_factory.mktemp("merge_inertial_ba_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"], "san")
    for name in ALL:
        assert mc.decisions(san[name][2]) == mc.decisions(host_results[name][2]), name
        assert mc.within(mc.differences(host_results[name][2], san[name][2], mc.scene(name)), mc.bounds()), name


def test_the_golden_file_is_current(measured):
    g = mc.golden()
    assert g["margin"] == mc.MARGIN and [tuple(v) for v in g["variants"]] == list(mc.VARIANTS) and tuple(sorted(g["scenes"])) == tuple(sorted(ALL))
    for q in mc.QUANTITIES:                                                    # the committed D is what --measure gives: never below it
        assert measured["D"][q] <= g["D"][q] and g["D"][q] <= 2 * measured["D"][q] + 1e-18, (q, measured["D"][q], g["D"][q])
    for name in ALL:
        m, s = measured["scenes"][name], g["scenes"][name]
        assert m["decisions"] == s["decisions"], name
        for key in ("decision_margin", "chi2_margin"):                         # what the fair-demand test reads is what --measure gives
            assert 0.5 * m[key] <= s[key] <= 2 * m[key], (name, key, m[key], s[key])
        assert sorted(m["movement"]) == sorted(s["movement"])
        for q, moved in s["movement"].items():
            assert 0.5 * m["movement"][q] <= moved <= 2 * m["movement"][q], (name, q, m["movement"][q], moved)


def test_the_scenes_make_equal_decisions_a_fair_demand(measured):
    g = mc.golden()
    assert measured["variants_agree"] and g["variants_agree"]
    b = mc.bounds()
    for name in ALL:
        for s in (g["scenes"][name], measured["scenes"][name]):                # as committed, and as measured now
            # no accept / reject decision of Levenberg and no classification within 100 times the scene's own spread
            assert s["decision_margin"] >= 100 * s["D"].get("cost", 0.0), (name, s["decision_margin"], s["D"])
            assert s["chi2_margin"] >= 100 * s["D"].get("chi2", 0.0), (name, s["chi2_margin"], s["D"])
            # every free vertex of every type and every point that is a vertex moves further than the bound of its quantity: a
            # block that was never updated cannot pass
            for q, moved in s["movement"].items():
                assert moved > b[q], (name, q, moved, b[q])
            assert bool(s["movement"]) == (s["decisions"][0] == 0)


def test_each_scene_is_what_it_is_named_for():
    sc, ref, G = mc.scene, mc.reference, (lambda n: mc.graph(mc.scene(n)))
    kinds = lambda n: [int((sc(n)["kf"]["kind"] == k).sum()) for k in range(4)]  # noqa: E731
    for n, counts, Kf, size in (("small", [5, 1, 0, 2], 7, 87), ("no_cov", [7, 1, 0, 0], 7, 105), ("pose_only_many", [3, 1, 0, 8], 11, 93),
                                ("fixed_pose_only", [5, 0, 1, 2], 7, 87), ("full", [13, 1, 0, 30], 43, 375)):
        assert kinds(n) == counts and (G(n)["Kf"], G(n)["n"]) == (Kf, size), n
        assert mc.validate(sc(n)) is None
    m = sc("small")["ur"] < 0
    assert m.any() and (~m).any() and len(sc("small")["pos"]) == 60
    chains = lambda s: len({int(E["pre"]["kf_prev"]) for E in s["ie"]} - {int(E["pre"]["kf_cur"]) for E in s["ie"]})  # noqa: E731
    assert chains(sc("small")) == 2 and chains(sc("broken_link")) == 3 and chains(sc("fixed_pose_only")) == 2
    s = sc("fixed_pose_only")                                                  # no link at the fixed KeyFrame: its chain starts free
    assert all(int(E["pre"]["kf_prev"]) != 0 for E in s["ie"]) and s["kf"]["kind"][1] == 0
    s, g, r = sc("idle_cov"), G("idle_cov"), ref("idle_cov")
    K, P = len(s["kf"]), len(s["pos"])
    assert s["kf"]["kind"][K - 1] == 3 and (s["edge_kf"] != K - 1).all() and g["free_of"][K - 1] < 0
    assert list(s["edge_kf"][s["edge_pt"] == P - 1]) == [0] and not g["included"][P - 1] and g["included"][:P - 1].all()
    assert r["status"] == 0 and np.array_equal(r["st"][K - 1]["Rwb"], s["kf"][K - 1]["Rwb"].reshape(3, 3)) and not r["flags"][-1]
    r = ref("outliers")
    assert sc("outliers")["iterations"] == 0 and r["iterations"] == 8 and r["rejected_trials"] >= 1 and r["flags"].any() and not r["flags"].all()
    # an edge whose point ends behind its camera with chi2 below the threshold is not flagged
    s, g, r = sc("depth_negative"), G("depth_negative"), ref("depth_negative")
    e = int(np.flatnonzero(s["edge_pt"] == 0)[0])
    k = int(s["edge_kf"][e])
    assert (s["edge_pt"] == 0).sum() == 1 and s["ur"][e] < 0 and g["free_of"][k] >= 0
    z = r["st"][k]["Rcw"][2] @ r["pts"][0] + r["st"][k]["tcw"][2]
    assert z < -1.0 and r["chi2"][e] < 0.5 * float(mc.CHI2_MONO) and not r["flags"][e] and r["flags"].any()
    assert (sc("mono_only")["ur"] < 0).all() and (sc("stereo_only")["ur"] >= 0).all()
    assert ref("stop_preset")["status"] == 3
    # the flag after a rejected trial: the loop of trials ends there, the flags belong to the rejected copy
    r = ref("stop_trial")
    assert (r["iterations"], r["trials"], r["rejected_trials"]) == (5, 5, 1) and ref("outliers")["trials"] == 9
    r = ref("stop_iteration")
    assert r["iterations"] == 2 and sc("stop_iteration")["iterations"] == 5
    for n in ALL:
        assert ref(n)["status"] == (3 if n == "stop_preset" else 0) and ref(n)["solver_failures"] == 0, n
        assert (sc(n)["kf"]["kind"] != 0).any() and ((sc(n)["kf"]["kind"] == 1) | (sc(n)["kf"]["kind"] == 2)).sum() == 1   # one fixed KeyFrame


def test_a_flag_that_rises_before_the_first_iteration_and_nothing_to_optimise():
    s = mc.scene("small")
    for kw in (dict(stop_trials=0), dict(stop_iteration=0)):
        r = mc.optimize(s, **kw)
        assert r["status"] == 3 and r["iterations"] == 0 and not r["included"].any() and not r["flags"].any()
    only_fixed = dict(s, kf=s["kf"].copy())
    only_fixed["kf"]["kind"] = 1
    assert mc.optimize(only_fixed)["status"] == 2
    no_edges = dict(s, ie=s["ie"][:0], edge_kf=s["edge_kf"][:0], edge_pt=s["edge_pt"][:0], xy=s["xy"][:0], ur=s["ur"][:0], inv=s["inv"][:0])
    assert mc.optimize(no_edges)["status"] == 2                                # free KeyFrames that no edge reaches are no vertices


def test_the_graphs_the_entry_refuses():
    s = mc.scene("small")
    ie = s["ie"].copy()
    ie[0]["pre"]["kf_cur"] = len(s["kf"]) - 1                                  # an inertial edge on a pose-only KeyFrame
    assert mc.validate(dict(s, ie=ie)) == "invalid"
    fork = np.concatenate([s["ie"], s["ie"][:1]])
    fork[-1]["pre"]["kf_cur"] = 3                                              # two edges leave one KeyFrame
    assert mc.validate(dict(s, ie=fork)) == "capacity"
    cyc = s["ie"][2:4].copy()                                                  # 3 -> 4 -> 5 closed by 5 -> 3
    extra = cyc[:1].copy()
    extra[0]["pre"]["kf_prev"], extra[0]["pre"]["kf_cur"] = 5, 3
    assert mc.validate(dict(s, ie=np.concatenate([cyc, extra]))) == "capacity"
