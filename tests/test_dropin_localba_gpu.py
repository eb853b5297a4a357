"""ms-slam_amd/host/Optimizer_device.h's LocalBundleAdjustment compiled against stand-in KeyFrame / MapPoint / Map types
(tests/dropin_localba_main.cc), linked to libmsorb.so through the C ABI and run on the GPU.  The program first checks the arrays
gathered from a covisibility graph listed by hand in its source.  Then, on a graph made from a scene of tests/local_ba_cases.py: the
gathered problem holds exactly the scene's edges, point-major, the local KeyFrames first; the erased observations, the poses, the
positions and mnOptimizedTimesInLBA after the call equal what the Python mirror returns for the gathered arrays; a KeyFrame with
a second camera makes the routine return false with nothing touched."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.dirname(os.path.abspath(__file__))]
import local_ba_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("localba") / "dropin_localba"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include",
                           f"{ROOT}/tests/dropin_localba_main.cc", f"-L{ROOT}/ms-slam_amd", "-lmsorb", f"-Wl,-rpath,{ROOT}/ms-slam_amd",
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", str(out)])
    return out


N_LEVELS = 8
INV_LEVEL = (1.0 / (1.2 ** np.arange(N_LEVELS)) ** 2).astype(np.float32)


def _write(path, s, init_id):
    kf = s["kf"]
    K, P, E = len(kf), len(s["pos_w"]), len(s["edge_kf"])
    octave = np.array([int(np.argmin(np.abs(INV_LEVEL - w))) for w in s["inv_sigma2"]], np.int32)
    assert np.array_equal(INV_LEVEL[octave], s["inv_sigma2"])
    local = (np.arange(K) < s["n_local"]).astype(np.int32)
    with open(path, "wb") as f:
        f.write(struct.pack("<iiiii", K, P, E, N_LEVELS, init_id))
        f.write(INV_LEVEL.astype("<f4").tobytes())
        for k in range(K):
            f.write(np.concatenate([kf["q"][k], kf["t"][k], [kf[c][k] for c in ("fx", "fy", "cx", "cy", "mbf")]]).astype("<f4").tobytes())
            f.write(struct.pack("<i", int(local[k])))
        f.write(s["pos_w"].astype("<f4").tobytes())
        for e in range(E):
            f.write(struct.pack("<iifffi", int(s["edge_kf"][e]), int(s["edge_point"][e]), *[float(v) for v in s["xy"][e]], float(s["u_right"][e]),
                                int(octave[e])))


def _read(blob, K, P, E):
    pos = 0

    def take(fmt, n=1):
        nonlocal pos
        a = np.frombuffer(blob, fmt, n, pos)
        pos += a.nbytes
        return a

    Kg, Pg, Eg = (int(v) for v in take("<i4", 3))
    kf_dt = np.dtype([("id", "<i4"), ("fixed", "<i4"), ("q", "<f4", 4), ("t", "<f4", 3)])
    e_dt = np.dtype([("kf", "<i4"), ("point", "<i4"), ("xy", "<f4", 2), ("ur", "<f4"), ("inv", "<f4")])
    g = dict(kf=take(kf_dt, Kg), point_id=take("<i4", Pg), edge=take(e_dt, Eg))
    ret = take("<i4", 5)
    after_kf = take(np.dtype([("qt", "<f4", 7), ("n_set_pose", "<i4")]), K)
    after_mp = take(np.dtype([("pos", "<f4", 3), ("times", "<i4"), ("n_update", "<i4")]), P)
    still = take(np.uint8, E).astype(bool)
    rig = take("<i4", 3)
    assert pos == len(blob)
    return g, ret, after_kf, after_mp, still, rig


def test_host_template(exe, tmp_path, msorb_mod):
    # 5 local KeyFrames of which KeyFrame 2 is the map's first (fixed = 1), 3 fixed cameras; every point is seen by a local KeyFrame
    s = lc.make_scene(301, free=5, fixed=3, points=120, degree=5, outliers=0.15)
    s["n_local"] = 5
    K, P, E = len(s["kf"]), len(s["pos_w"]), len(s["edge_kf"])
    local_edge = s["edge_kf"] < 5
    assert all(local_edge[s["edge_point"] == p].any() for p in range(P))
    _write(tmp_path / "in.bin", s, init_id=10 + 2)
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    g, ret, after_kf, after_mp, still, rig = _read((tmp_path / "out.bin").read_bytes(), K, P, E)
    # ---- the gathered problem: the scene's KeyFrames (local first, the InitKFid one and the cameras fixed), points and edges
    ids = g["kf"]["id"] - 10
    assert sorted(ids.tolist()) == list(range(K)) and set(ids[:5].tolist()) == set(range(5)) and ids[0] == 0
    assert np.array_equal(g["kf"]["fixed"], ((ids >= 5) | (ids == 2)).astype(np.int32))
    assert np.array_equal(g["kf"]["q"], s["kf"]["q"][ids]) and np.array_equal(g["kf"]["t"], s["kf"]["t"][ids])
    pid = g["point_id"] - 500
    assert sorted(pid.tolist()) == list(range(P)) + [402]           # the point whose only observation is at octave 11
    ge = g["edge"]
    assert (np.diff(ge["point"]) >= 0).all() and len(ge) == E
    got = sorted(zip(ids[ge["kf"]].tolist(), pid[ge["point"]].tolist(), ge["xy"][:, 0].tolist(), ge["xy"][:, 1].tolist(), ge["ur"].tolist(),
                     ge["inv"].tolist()))
    want = sorted(zip(s["edge_kf"].tolist(), s["edge_point"].tolist(), s["xy"][:, 0].tolist(), s["xy"][:, 1].tolist(),
                      s["u_right"].tolist(), s["inv_sigma2"].tolist()))
    assert got == want
    # ---- the call: what the C ABI returns for the gathered arrays
    kfs = msorb_mod.ba_keyframes(g["kf"]["q"], g["kf"]["t"], {k: np.float32(v) for k, v in lc.pc.KITTI.items()}, g["kf"]["fixed"])
    pos_w = np.concatenate([s["pos_w"], np.array([[2, 1, 14]], np.float32)])[np.where(pid == 402, P, pid)]
    r = msorb_mod.local_ba(kfs, pos_w, ge["kf"], ge["point"], ge["xy"], ge["ur"], ge["inv"])
    res = r["result"]
    assert res["status"] == 0 and res["iterations"] > 0 and 0 < res["n_outliers"] < E
    assert ret.tolist() == [1, 4, 5, E, 1]                          # true; 3 cameras + the InitKFid KeyFrame; 5 local; the edges; one change
    # erased observations = the flagged edges
    flagged = {(int(ids[ge["kf"][e]]), int(pid[ge["point"][e]])) for e in np.nonzero(r["outlier"])[0]}
    erased = {(int(s["edge_kf"][e]), int(s["edge_point"][e])) for e in np.nonzero(~still)[0]}
    assert erased == flagged
    # SetPose for every local KeyFrame (the fixed one too, :1388-1395) with the narrowed estimate, nothing for the cameras
    for row, k in enumerate(ids):
        if row < 5:
            assert after_kf["n_set_pose"][k] == 1 and after_kf["qt"][k].tobytes() == r["kf_qt"][row].tobytes()
        else:
            assert after_kf["n_set_pose"][k] == 0
            assert after_kf["qt"][k].tobytes() == np.concatenate([s["kf"]["q"][k], s["kf"]["t"][k]]).tobytes()
    moved = np.abs(r["kf_qt"][:5, 4:] - g["kf"]["t"][:5]).max(1)
    assert (moved[g["kf"]["fixed"][:5] == 0] > 0).all() and (moved[g["kf"]["fixed"][:5] == 1] == 0).all()
    # SetWorldPos, UpdateNormalAndDepth, mnOptimizedTimesInLBA++ for every local point
    for row, p in enumerate(pid):
        if p < P:
            assert after_mp["pos"][p].tobytes() == r["pos"][row].tobytes()
    assert (after_mp["times"] == 1).all() and (after_mp["n_update"] == 1).all()
    # ---- a KeyFrame with a second camera: false, no SetPose, no counter, no mark, no change index
    assert rig.tolist() == [0, 0, 0]
