"""msorb_host::FullInertialBA (ms-slam_amd/host/Optimizer_device.h) compiled over stand-in KeyFrame / MapPoint / Map /
IMU::Preintegrated types (tests/dropin_full_inertial_ba_main.cc) and linked to the library.

CPU: the gathering on a graph listed by hand in the program, in both forms (kinds under bFixLocal, the order of the unknowns against
the order of the map's list, the links and their SetNewBias list, pIncKF's biases, the octave > 10 skip, a KeyFrame above maxKFid),
bFixLocal's nNonFixed < 3 return, and every "not handled" case (a second camera, a free KeyFrame without bImu, two KeyFrames with one
mPrevKF, a link without preintegration): false, with no setter, no SetNewBias and no change index left behind.

GPU: two scenes of tests/full_inertial_ba_cases.py per write-back arm as a stand-in map.  The gathered problem equals the scene;
every setter (nLoopId == 0) or *GBA member (otherwise) received the bits the Python mirror returns for the gathered problem;
mnBAGlobalForKF is set only in the loop arm; IncreaseChangeIndex ran once; every link's preintegration received one SetNewBias."""
import os
import subprocess

import numpy as np
import pytest

import full_inertial_ba_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dropin_full_inertial_ba") / "dropin_full_inertial_ba")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include",
                           f"{ROOT}/tests/dropin_full_inertial_ba_main.cc", f"-L{ROOT}/ms-slam_amd", "-lmsorb", f"-Wl,-rpath,{ROOT}/ms-slam_amd",
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def test_hand_listed_graph_and_refusals(exe):
    p = subprocess.run([exe, "--hand"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr[-2000:])


@pytest.mark.gpu
@pytest.mark.parametrize("name,loop_id", [("f4", 0), ("i10", 0), ("two_chains", 7), ("mixed", 7)])
def test_template_over_a_scene(msorb_mod, exe, tmp_path, name, loop_id):
    sc = fc.scene(name)
    K, P = len(sc["kf"]), len(sc["pos"])
    fc.write_dropin_scene(str(tmp_path / "in.bin"), sc, loop_id)
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr[-2000:])
    g, r = fc.read_dropin_result(str(tmp_path / "out.bin"), sc)
    # ---- the gathered problem against the scene
    assert (g["init"], g["iterations"]) == (sc["init"], sc["iterations"]) and g["prior_g"] == sc["prior_g"] and g["prior_a"] == sc["prior_a"]
    assert np.array_equal(g["kf"]["kind"], sc["kf"]["kind"])
    for k in ("Rwb", "twb", "v", "bg", "ba", "Rcw", "tcw", "tbc", "fx", "fy", "cx", "cy", "mbf"):
        assert np.array_equal(g["kf"][k], sc["kf"][k]), k                      # floats widened: exact
    for k in ("Rcb", "tcb"):                                                   # the stand-in's mTcb is float, the scene's double
        assert np.allclose(g["kf"][k], sc["kf"][k], rtol=0, atol=1e-7), k
    # the map lists its KeyFrames newest first: the links come in that order; huber on every edge, no downweight
    want = sorted(((int(e["pre"]["kf_prev"]), int(e["pre"]["kf_cur"])) for e in sc["ie"]), key=lambda t: -t[1])
    assert [(int(e["pre"]["kf_prev"]), int(e["pre"]["kf_cur"])) for e in g["ie"]] == want
    assert g["ie"]["huber"].all() and not g["ie"]["downweight"].any()
    by_cur = {int(e["pre"]["kf_cur"]): e for e in sc["ie"]}
    for e in g["ie"]:
        s = by_cur[int(e["pre"]["kf_cur"])]
        for k in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "bias", "dT"):
            assert np.array_equal(e["pre"][k], s["pre"][k]), k
        assert np.abs(e["pre"]["info"] - s["pre"]["info"]).max() <= 1e-5 * np.abs(s["pre"]["info"]).max()   # the project's Jacobi against numpy's eigh
        if not sc["init"]:
            assert np.allclose(e["info_gyro"], s["info_gyro"], rtol=1e-9) and np.allclose(e["info_acc"], s["info_acc"], rtol=1e-9)
    if sc["init"]:                                                             # pIncKF is the last of the map's list: KeyFrame 0
        assert np.array_equal(g["bg0"], sc["kf"]["bg"][0]) and np.array_equal(g["ba0"], sc["kf"]["ba"][0])
    for k in ("pos", "edge_kf", "edge_pt", "xy", "ur", "inv"):
        assert np.array_equal(g[k], sc[k]), k
    # ---- what the setters received against the Python mirror on the gathered problem
    out = msorb_mod.full_inertial_ba(g["kf"], g["ie"], g["pos"], g["edge_kf"], g["edge_pt"], g["xy"], g["ur"], g["inv"], init=bool(g["init"]),
                                     iterations=g["iterations"], prior_g=g["prior_g"], prior_a=g["prior_a"], bg0=g["bg0"], ba0=g["ba0"])
    assert int(out["result"]["status"]) == 0 and int(out["result"]["iterations"]) >= 1
    assert r["ret"] == 1 and r["change"] == 1 and r["n_new_bias"] == len(sc["ie"])
    kf, pts, inc = r["kf"], r["pts"], out["included"]
    arm = "" if loop_id == 0 else "_gba"
    assert np.array_equal(kf["Rcw" + arm], out["kf"]["Rcw_f"]) and np.array_equal(kf["tcw" + arm], out["kf"]["tcw_f"])
    assert np.array_equal(kf["v" + arm], out["kf"]["v_f"]) and np.array_equal(kf["bias" + arm], out["kf"]["bias_f"])
    assert not np.array_equal(out["kf"]["tcw_f"], sc["kf"]["tcw"].astype(np.float32))          # (something moved)
    assert np.array_equal(pts["pos" + arm][inc], out["pos"][inc]) and inc.sum() >= P - 1
    if loop_id == 0:
        assert (kf["n_set_pose"] == 1).all() and (kf["n_set_velocity"] == 1).all() and (kf["n_set_bias"] == 1).all() and (kf["gba_mark"] == 0).all()
        assert np.array_equal(pts["n_set_pos"], inc.astype(np.int32)) and np.array_equal(pts["n_update"], inc.astype(np.int32)) and (pts["gba_mark"] == 0).all()
        assert not kf["Rcw_gba"][:, 1].any() and not pts["pos_gba"].any()                        # the loop arm's members untouched
    else:
        assert not kf["n_set_pose"].any() and not kf["n_set_velocity"].any() and not kf["n_set_bias"].any() and (kf["gba_mark"] == loop_id).all()
        assert not pts["n_set_pos"].any() and not pts["n_update"].any() and np.array_equal(pts["gba_mark"], loop_id * inc.astype(np.int32))
        assert np.array_equal(kf["tcw"], sc["kf"]["tcw"].astype(np.float32)) and np.array_equal(pts["pos"], sc["pos"])   # the estimates untouched
