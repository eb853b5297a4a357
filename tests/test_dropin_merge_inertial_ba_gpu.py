"""msorb_host::MergeInertialBA (ms-slam_amd/host/Optimizer_device.h) compiled over stand-in KeyFrame / MapPoint / Map /
IMU::Preintegrated / g2o::Sim3 types (tests/dropin_merge_inertial_ba_main.cc) and linked to the library.

CPU: the gathering on two graphs listed by hand in the program: both temporal windows with mNextKF, the covisible KeyFrame before
the current window, the fixed KeyFrame before the merge window, and both pop_back arms (:3946-3949, :3968-3973); the sort by
observation count together with the maxCovKF cut (a KeyFrame that sees only a point behind the cut is not gathered; without the
sort it would be); the octave > 10 skip; the kinds by g2o's active set; the order of the unknowns and of the inertial edges.  Every
"not handled" case (a second camera, a link without preintegration or without bImu, a gathered KeyFrame above maxKFid, maxKFid <= 2,
one KeyFrame gathered twice) returns false with no setter called, no SetNewBias and every mark as it was; the flag found set returns
true with the marks and the SetNewBias of :4142 alone.  (An observation by a KeyFrame above maxKFid, :4250, can only belong to a
KeyFrame that was gathered, which is not handled, or to one without a mark, which :4247 skips first.)

GPU: two scenes of tests/merge_inertial_ba_cases.py as stand-in maps.  The gathered problem equals the scene; every setter, every
corrPoses entry and every erased observation received the bits the Python mirror returns for the gathered problem;
IncreaseChangeIndex ran once; every link's preintegration received one SetNewBias.  reserved != 0 and a flag that rises between the
gathering and the first iteration cannot be produced on demand: their arm is the one line that tests status and reserved."""
import os
import subprocess

import numpy as np
import pytest

import merge_inertial_ba_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dropin_merge_inertial_ba") / "dropin_merge_inertial_ba")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include",
                           f"{ROOT}/tests/dropin_merge_inertial_ba_main.cc", f"-L{ROOT}/ms-slam_amd", "-lmsorb", f"-Wl,-rpath,{ROOT}/ms-slam_amd",
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def test_hand_listed_graphs_and_refusals(exe):
    p = subprocess.run([exe, "--hand"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr[-2000:])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "outliers"])
def test_template_over_a_scene(msorb_mod, exe, tmp_path, name):
    sc, curr, merge = mc.dropin_scene(mc.scene(name))
    K, P, E = len(sc["kf"]), len(sc["pos"]), len(sc["edge_kf"])
    mc.write_dropin_scene(str(tmp_path / "in.bin"), sc, curr, merge)
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr[-2000:])
    g, r = mc.read_dropin_result(str(tmp_path / "out.bin"), sc)
    # ---- the gathered problem against the scene
    assert g["iterations"] == 0 and np.array_equal(g["kf"]["kind"], sc["kf"]["kind"])
    for k in ("Rwb", "twb", "v", "bg", "ba", "Rcw", "tcw", "tbc", "fx", "fy", "cx", "cy", "mbf"):
        assert np.array_equal(g["kf"][k], sc["kf"][k]), k                      # floats widened: exact
    for k in ("Rcb", "tcb"):                                                   # the stand-in's mTcb is float, the scene's double
        assert np.allclose(g["kf"][k], sc["kf"][k], rtol=0, atol=1e-7), k
    # the links in the order of the loop over vpOptimizableKFs: each window newest first, the current one before the merge one
    links = lambda ie: [(int(e["pre"]["kf_prev"]), int(e["pre"]["kf_cur"])) for e in ie]  # noqa: E731
    assert links(g["ie"]) == sorted(links(sc["ie"]), key=lambda t: -t[1])
    assert g["ie"]["huber"].all() and not g["ie"]["downweight"].any()
    by_cur = {int(e["pre"]["kf_cur"]): e for e in sc["ie"]}
    for e in g["ie"]:
        s = by_cur[int(e["pre"]["kf_cur"])]
        for k in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "bias", "dT"):
            assert np.array_equal(e["pre"][k], s["pre"][k]), k
        assert np.abs(e["pre"]["info"] - s["pre"]["info"]).max() <= 1e-5 * np.abs(s["pre"]["info"]).max()   # the project's Jacobi against numpy's eigh
        assert np.allclose(e["info_gyro"], s["info_gyro"], rtol=1e-9) and np.allclose(e["info_acc"], s["info_acc"], rtol=1e-9)
    # the points come in the order the window KeyFrames list them: every point once, and each point's edges as the scene has them
    ids = g["point_ids"]
    assert sorted(ids) == list(range(P)) and np.array_equal(g["pos"], sc["pos"][ids])
    scene_edge = {}                                                            # gathered edge -> the scene's edge
    first = np.searchsorted(sc["edge_pt"], np.arange(P + 1))
    at = 0
    for q, pid in enumerate(ids):
        n = first[pid + 1] - first[pid]
        assert (g["edge_pt"][at:at + n] == q).all() and (at + n == len(g["edge_pt"]) or g["edge_pt"][at + n] != q)
        for j in range(n):
            scene_edge[at + j] = first[pid] + j
        at += n
    assert at == E == len(g["edge_kf"])
    to_scene = np.array([scene_edge[e] for e in range(E)])
    for k in ("edge_kf", "xy", "ur", "inv"):
        assert np.array_equal(g[k], sc[k][to_scene]), k
    # ---- what the setters received against the Python mirror on the gathered problem
    out = msorb_mod.merge_inertial_ba(g["kf"], g["ie"], g["pos"], g["edge_kf"], g["edge_pt"], g["xy"], g["ur"], g["inv"])
    res = out["result"]
    assert int(res["status"]) == 0 and int(res["iterations"]) >= 1 and int(res["reserved"]) == 0 and out["included"].all()
    assert r["ret"] == 1 and r["change"] == 1 and r["n_new_bias"] == len(sc["ie"])
    kf, kind = r["kf"], sc["kf"]["kind"]
    free = (kind == 0) | (kind == 3)
    assert np.array_equal(kf["n_set_pose"], free.astype(np.int32)) and np.array_equal(kf["has_corr"], free.astype(np.int32))
    assert np.array_equal(kf["n_set_velocity"], free.astype(np.int32)) and np.array_equal(kf["n_set_bias"], free.astype(np.int32))   # (every KeyFrame has bImu)
    assert np.array_equal(kf["Rcw"][free], out["kf"]["Rcw_f"][free]) and np.array_equal(kf["tcw"][free], out["kf"]["tcw_f"][free])
    assert np.array_equal(kf["v"][free], out["kf"]["v_f"][free]) and np.array_equal(kf["bias"][free], out["kf"]["bias_f"][free])
    assert not np.array_equal(out["kf"]["tcw_f"][free], sc["kf"]["tcw"].astype(np.float32)[free])          # (something moved)
    # corrPoses: the pose the setter received, widened, with scale 1
    assert np.array_equal(kf["corr_R"][free], kf["Rcw"][free].astype(np.float64)) and np.array_equal(kf["corr_t"][free], kf["tcw"][free].astype(np.float64))
    assert (kf["corr_s"][free] == 1.0).all() and not kf["corr_s"][~free].any()
    fixed = ~free                                                              # the fixed KeyFrame: untouched
    assert np.array_equal(kf["tcw"][fixed], sc["kf"]["tcw"].astype(np.float32)[fixed])
    pts = r["pts"]
    assert (pts["n_set_pos"] == 1).all() and (pts["n_update"] == 1).all() and np.array_equal(pts["pos"][ids], out["pos"])
    # the erased observations are the flagged edges
    erased = np.zeros(E, bool)
    erased[to_scene] = out["outlier"]
    assert np.array_equal(~r["still"], erased)
    if name == "outliers":
        assert erased.any() and not erased.all()
