"""msorb_host::CreateNewMapPoints (ms-slam_amd/host/LocalMapping_device.h) compiled against the stand-ins of tests/slam_stub
(tests/dropin_newpoints_main.cc) and driven like LocalMapping::CreateNewMapPoints drives the reference's loop: the sequence of
onNewPoint calls (neighbour, idx1, idx2, the bits of x3D) against R32 of tests/new_map_points_cases.py, fed with the camera centres,
F12 and epipoles the C++ side computed (the Sophus / Eigen arithmetic there is the caller's code)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import new_map_points_cases as nmp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPPED = 2     # this neighbour sits 0.1 from the current KeyFrame: less than its mb, the baseline test of :476 drops it


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("dropin_newpoints") / "dropin_newpoints"
    subprocess.check_call(["g++", "-std=c++17", "-O2", f"-I{ROOT}/tests/slam_stub", f"-I{ROOT}/tests/cv_stub", f"-I{ROOT}/ms-slam_amd/host",
                           f"-I{ROOT}/include", f"{ROOT}/tests/dropin_newpoints_main.cc", f"-L{ROOT}/ms-slam_amd", "-lmsorb",
                           f"-Wl,-rpath,{ROOT}/ms-slam_amd", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def scene(oracle):
    sc = nmp.make_scene(41, n1=150, K=4, n2=140, check_orientation=False, th_far=60.0, inertial=True)
    g0, g = sc["kfs"][0]["geometry"], sc["kfs"][DROPPED + 1]["geometry"]
    R = g["Tcw"][:, :3].astype(np.float64)
    g["Tcw"][:, 3] = (-R @ (g0["Ow"].astype(np.float64) + [0.1, 0, 0])).astype(np.float32)
    return sc


def _scene_file(sc):
    K = len(sc["kfs"]) - 1
    out = [struct.pack("<iiiif", K, int(sc["coarse"]), int(sc["inertial"]), int(sc["th_far"] > 0), float(sc["th_far"]))]
    for k, kf in enumerate(sc["kfs"]):
        n, g = len(kf["kps"]), kf["geometry"]
        node = -np.ones(n, np.int32)
        nodes, begin, feat = kf["fv"]
        for r, nd in enumerate(nodes):
            node[feat[begin[r]:begin[r + 1]]] = nd
        free_ = sc["valid1"] if k == 0 else sc["avail2"][k - 1]
        out += [struct.pack("<i", n), np.ascontiguousarray(kf["kps"]).tobytes(), kf["desc"].tobytes(), g["u_right"].tobytes(),
                g["depth"].tobytes(), node.tobytes(), (1 - free_).astype(np.uint8).tobytes(),
                np.ascontiguousarray(g["Tcw"][:, :3]).tobytes(), np.ascontiguousarray(g["Tcw"][:, 3]).tobytes(),
                np.array([g[q] for q in ("fx", "fy", "cx", "cy", "mb", "mbf")], np.float32).tobytes()]
    out += [nmp.SCALE.tobytes() + nmp.SIGMA2.tobytes()] * (K + 1)
    return b"".join(out)


def _run(exe, tmp_path, sc, stop_before=-1, rig=0):
    fin, fout = str(tmp_path / "scene.bin"), str(tmp_path / "log.bin")
    with open(fin, "wb") as f:
        f.write(_scene_file(sc))
    subprocess.check_call([exe, fin, fout, str(stop_before), str(rig)], timeout=120)
    raw = open(fout, "rb").read()
    K = len(sc["kfs"]) - 1
    ret, n_log = struct.unpack_from("<ii", raw)
    geo = np.frombuffer(raw, np.float32, 14 * (K + 1), 8).reshape(K + 1, 14)
    log = np.frombuffer(raw, np.uint32, 6 * n_log, 8 + 56 * (K + 1)).reshape(n_log, 6)
    return ret, geo, log


def _expected(sc, geo, neighbours):
    """R32 over the neighbours the baseline test keeps, with the C++ side's camera centres, F12 and epipoles -> the log"""
    ref = dict(sc)
    ref["kfs"] = [dict(sc["kfs"][k], geometry=dict(sc["kfs"][k]["geometry"], Ow=geo[k, 11:14].copy())) for k in [0] + [i + 1 for i in neighbours]]
    ref["avail2"] = [sc["avail2"][i] for i in neighbours]
    ref["F12"] = [geo[i + 1, :9].reshape(3, 3).copy() for i in neighbours]
    ref["ep"] = [geo[i + 1, 9:11].copy() for i in neighbours]
    rows = []
    for i, r in zip(neighbours, nmp.R32(ref)):
        for idx1 in np.nonzero((r["status"] >= nmp.TRIANGULATED) & (r["status"] <= nmp.STEREO2))[0]:
            rows.append([i, idx1, r["match12"][idx1], *r["x3D"][idx1].view(np.uint32)])
    return np.array(rows, np.uint32).reshape(-1, 6)


def test_template_reports_the_reference_sequence(exe, scene, tmp_path):
    ret, geo, log = _run(exe, tmp_path, scene)
    want = _expected(scene, geo, [0, 1, 3])
    assert ret == 1 and len(want) > 40 and len(set(want[:, 0])) == 3
    assert np.array_equal(log, want)


def test_a_new_keyframe_stops_the_walk(exe, scene, tmp_path):
    ret, geo, log = _run(exe, tmp_path, scene, stop_before=2)
    want = _expected(scene, geo, [0, 1, 3])
    assert ret == 1 and np.array_equal(log, want[want[:, 0] < 2]) and len(log) > 0


def test_a_second_camera_is_left_to_the_caller(exe, scene, tmp_path):
    ret, _, log = _run(exe, tmp_path, scene, rig=1)
    assert ret == 0 and len(log) == 0
