"""msorb_host::LocalInertialBA (ms-slam_amd/host/Optimizer_device.h) compiled over stand-in KeyFrame / MapPoint / Map /
IMU::Preintegrated types (tests/dropin_local_inertial_ba_main.cc) and linked to the library.

CPU: the gathering on a graph listed by hand in the program (kinds, chain order, the Huber / downweight flags for bRecInit 0 and 1,
the octave > 10 skip, the arm without mPrevKF) and the refusals (a second camera on an observer or on a window KeyFrame, a window
KeyFrame or the KeyFrame before the window with !bImu: false, no mark, no SetNewBias, no change index).

GPU: a scene of tests/local_inertial_ba_cases.py as a stand-in graph.  The gathered problem equals the scene where the reference's
walk keeps it (it makes at most ONE new fixed KeyFrame per local point, :2526-2531, so some observers of the scene stay out);
every setter received the bits the Python mirror returns for the gathered problem; the erased observations are the flagged edges.
No scene reaches status 1 (tests/test_local_inertial_ba_cpu.py), so "nothing written on FAIL" is not run here."""
import os
import subprocess

import numpy as np
import pytest

import local_inertial_ba_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dropin_local_inertial_ba") / "dropin_local_inertial_ba")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include",
                           f"{ROOT}/tests/dropin_local_inertial_ba_main.cc", f"-L{ROOT}/ms-slam_amd", "-lmsorb", f"-Wl,-rpath,{ROOT}/ms-slam_amd",
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


def test_hand_listed_graph_and_refusals(exe):
    p = subprocess.run([exe, "--hand"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr[-2000:])


@pytest.mark.gpu
@pytest.mark.parametrize("name,rec_init,no_prev", [("mixed", 0, 0), ("rec_init", 1, 0), ("no_prev", 0, 1), ("outliers", 0, 0)])
def test_template_over_a_scene(msorb_mod, exe, tmp_path, name, rec_init, no_prev):
    sc = lc.scene(name)
    K, P = len(sc["kf"]), len(sc["pos"])
    lc.write_dropin_scene(str(tmp_path / "in.bin"), sc, rec_init, no_prev)
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr[-2000:])
    g, r = lc.read_dropin_result(str(tmp_path / "out.bin"), sc)
    # ---- the gathered problem against the scene
    kfi = g["kf_ids"] - 10                                                     # scene index of every gathered KeyFrame, ascending mnId
    pti = g["point_ids"] - 500
    assert np.all(np.diff(kfi) > 0) and len(set(pti)) == len(pti)
    free = np.flatnonzero(sc["kf"]["kind"] == 0)
    assert set(free) <= set(kfi) and 0 in kfi                                  # the window and the KeyFrame before it (or without mPrevKF)
    assert np.array_equal(g["kf"]["kind"], sc["kf"]["kind"][kfi])
    for k in ("Rwb", "twb", "v", "bg", "ba", "Rcw", "tcw", "tbc", "fx", "fy", "cx", "cy", "mbf"):
        assert np.array_equal(g["kf"][k], sc["kf"][k][kfi]), k                 # floats widened: exact
    for k in ("Rcb", "tcb"):                                                   # the stand-in's mTcb is float, the scene's double
        assert np.allclose(g["kf"][k], sc["kf"][k][kfi], rtol=0, atol=1e-7), k
    n = len(free)
    pos_of = {int(s): i for i, s in enumerate(kfi)}
    assert len(g["ie"]) == n
    for i, e in enumerate(g["ie"]):                                            # the reference's loop runs from the newest KeyFrame
        cur = n - i
        assert (int(e["pre"]["kf_prev"]), int(e["pre"]["kf_cur"])) == (pos_of[cur - 1], pos_of[cur])
        assert int(e["huber"]) == int(i == n - 1 or bool(rec_init)) and int(e["downweight"]) == int(i == n - 1)
        s = sc["ie"][cur - 1]
        for k in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "bias", "dT"):
            assert np.array_equal(e["pre"][k], s["pre"][k]), k
        scale = np.abs(s["pre"]["info"]).max()
        assert np.abs(e["pre"]["info"] - s["pre"]["info"]).max() <= 1e-5 * scale          # the project's Jacobi against numpy's eigh
        assert np.allclose(e["info_gyro"], s["info_gyro"], rtol=1e-9) and np.allclose(e["info_acc"], s["info_acc"], rtol=1e-9)
    seen_by_window = np.isin(np.arange(P), sc["edge_pt"][np.isin(sc["edge_kf"], free) | ((sc["edge_kf"] == 0) & bool(no_prev))])
    assert set(pti) == set(np.flatnonzero(seen_by_window))                     # the local points: those the window's KeyFrames match
    assert np.array_equal(g["pos"], sc["pos"][pti]) and np.array_equal(g["close"], sc["close"][pti])
    keep = np.isin(sc["edge_kf"], kfi) & np.isin(sc["edge_pt"], pti)
    want = sorted(zip(sc["edge_pt"][keep].tolist(), sc["edge_kf"][keep].tolist(), sc["xy"][keep, 0].tolist(), sc["xy"][keep, 1].tolist(),
                      sc["ur"][keep].tolist(), sc["inv"][keep].tolist()))
    got = sorted(zip(pti[g["edge_pt"]].tolist(), kfi[g["edge_kf"]].tolist(), g["xy"][:, 0].tolist(), g["xy"][:, 1].tolist(), g["ur"].tolist(),
                     g["inv"].tolist()))
    assert got == want
    assert np.all(np.diff(g["edge_pt"]) >= 0)                                  # point-major
    # ---- the setters against the mirror on the gathered problem
    out = msorb_mod.local_inertial_ba(g["kf"], g["ie"], g["pos"], g["close"], g["edge_kf"], g["edge_pt"], g["xy"], g["ur"], g["inv"],
                                      large=bool(g["large"]), iterations=0)
    assert r["ret"] == 1 and int(out["result"]["status"]) == 0 and r["change"] == 1 and r["n_new_bias"] == n
    for j, s in enumerate(kfi):
        kf, o = r["kf"][s], out["kf"][j]
        if sc["kf"]["kind"][s] == 0:
            assert (kf["n_set_pose"], kf["n_set_velocity"], kf["n_set_bias"]) == (1, 1, 1)
            assert kf["Rcw"].tobytes() == o["Rcw_f"].tobytes() and kf["tcw"].tobytes() == o["tcw_f"].tobytes()
            assert kf["v"].tobytes() == o["v_f"].tobytes() and kf["bias"].tobytes() == o["bias_f"].tobytes()
            assert kf["local"] == 0
        else:
            assert (kf["n_set_pose"], kf["n_set_velocity"], kf["n_set_bias"]) == (0, 0, 0) and kf["fixed"] == 0
    others = np.setdiff1d(np.arange(K), kfi)
    assert not r["kf"]["n_set_pose"][others].any()
    for j, s in enumerate(pti):
        assert (r["pts"]["n_set_pos"][s], r["pts"]["n_update"][s]) == (1, 1) and r["pts"]["pos"][s].tobytes() == out["pos"][j].tobytes()
    assert not r["pts"]["n_set_pos"][np.setdiff1d(np.arange(P), pti)].any()
    # ---- the erased observations are the flagged edges
    flagged = set(zip(pti[g["edge_pt"]][out["outlier"]].tolist(), kfi[g["edge_kf"]][out["outlier"]].tolist()))
    erased = set(zip(sc["edge_pt"][~r["still"]].tolist(), sc["edge_kf"][~r["still"]].tolist()))
    assert erased == flagged and (name != "outliers" or len(flagged) > 10)
