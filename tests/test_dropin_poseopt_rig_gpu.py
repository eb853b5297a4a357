"""ms-slam_amd/host/Optimizer_device.h's PoseOptimizationAnyCamera compiled against stand-in Frame / MapPoint / GeometricCamera types
(tests/dropin_poseopt_rig_main.cc), linked to libmsorb.so through the C ABI and run on the GPU: a two-camera frame and a one-camera
fisheye frame give the mvbOutlier, the pose SetPose received and the return value the Python mirror computes on the same data; a
pinhole frame takes the old path; fewer than three points return 0 with the pose alone; an unknown camera type and a stereo
observation on a fisheye frame come back untouched with -1."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.dirname(os.path.abspath(__file__))]
import pose_opt_cases as pc  # noqa: E402
import pose_opt_rig_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu
N_LEVELS = 8
INV_LEVEL = (1.0 / (1.2 ** np.arange(N_LEVELS)) ** 2).astype(np.float32)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("poseopt_rig") / "dropin_poseopt_rig"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include",
                           f"{ROOT}/tests/dropin_poseopt_rig_main.cc", f"-L{ROOT}/ms-slam_amd", "-lmsorb", f"-Wl,-rpath,{ROOT}/ms-slam_amd",
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", str(out)])
    return out


def _frame(seed, xy, camera, pos_w, n_keys, two):
    """n_keys entries (the first half the left camera's when `two`) of which len(xy) carry the observations, in order; every 7th of
    the others carries a bad map point, the rest none -> per-entry arrays, the observations' weights, Nleft"""
    rng = np.random.default_rng(seed + 1000)
    n = len(xy)
    n_left = n_keys // 2 if two else n_keys
    cam = np.asarray(camera).astype(bool)
    slots = np.empty(n, np.int64)
    slots[~cam] = np.sort(rng.choice(n_left, int((~cam).sum()), replace=False))
    if cam.any():
        slots[cam] = n_left + np.sort(rng.choice(n_keys - n_left, int(cam.sum()), replace=False))
    assert np.all(np.diff(slots) > 0)                       # the gathering loop meets the observations in the scene's order
    octave = rng.integers(0, N_LEVELS, n_keys).astype(np.int32)
    x = rng.uniform(0, rc.IMAGE, n_keys).astype(np.float32)
    y = rng.uniform(0, rc.IMAGE, n_keys).astype(np.float32)
    ur = np.full(n_keys, -1, np.float32)
    pos = rng.uniform(-10, 10, (n_keys, 3)).astype(np.float32)
    state = np.where(np.arange(n_keys) % 7 == 0, 2, 0).astype(np.int32)
    x[slots], y[slots], pos[slots], state[slots] = xy[:, 0], xy[:, 1], pos_w, 1
    return dict(x=x, y=y, ur=ur, octave=octave, state=state, pos=pos, slots=slots), INV_LEVEL[octave[slots]], n_left


def _write(path, q, t, q_rl, t_rl, pin, cams, k, n_left):
    par = np.zeros((2, 8), np.float32)
    types = [0, 0]
    for c, (kind, p) in enumerate(cams):
        types[c] = kind
        par[c, :len(p)] = p
    if q_rl is None:
        q_rl, t_rl = np.array([0, 0, 0, 1], np.float32), np.zeros(3, np.float32)
    with open(path, "wb") as f:
        f.write(np.concatenate([q, t, q_rl, t_rl, np.asarray(pin, np.float32)]).astype("<f4").tobytes())
        f.write(struct.pack("<iii", len(cams), *types))
        f.write(par.astype("<f4").tobytes())
        f.write(struct.pack("<iii", len(k["x"]), n_left, N_LEVELS))
        f.write(INV_LEVEL.astype("<f4").tobytes())
        for i in range(len(k["x"])):
            f.write(struct.pack("<fffiifff", k["x"][i], k["y"][i], k["ur"][i], k["octave"][i], k["state"][i], *k["pos"][i]))


def _read(blob, n_keys):
    runs, pos = [], 0
    while pos < len(blob):
        ret, n_set = struct.unpack_from("<ii", blob, pos)
        pose = np.frombuffer(blob, "<f4", 7, pos + 8)
        flags = np.frombuffer(blob, np.uint8, n_keys, pos + 36).astype(bool)
        runs.append((ret, n_set, pose, flags))
        pos += 36 + n_keys
    return runs


def _run(exe, tmp_path, *args):
    _write(tmp_path / "in.bin", *args)
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    return _read((tmp_path / "out.bin").read_bytes(), len(args[-2]["x"]))


def _rig_case(seed, n_points, n_keys, cams):
    s = rc.make_rig_scene(seed, n_points, cams=cams, outliers=0.2, rot_deg=1.5, trans=0.08)
    k, inv, n_left = _frame(seed, s["xy"], s["camera"], s["pos_w"], n_keys, len(cams) == 2)
    s["inv_sigma2"] = inv                                   # the scene's weights become the frame's level table
    return s, k, n_left


@pytest.mark.parametrize("seed,n_points,n_keys,cams", [(51, 700, 1900, ("kb8", "kb8")), (52, 500, 1300, ("kb8",)), (53, 2, 60, ("kb8", "kb8"))])
def test_rig_and_fisheye_frames(exe, tmp_path, msorb_mod, seed, n_points, n_keys, cams):
    s, k, n_left = _rig_case(seed, n_points, n_keys, cams)
    (ret, n_set, pose, flags), = _run(exe, tmp_path, s["q"], s["t"], s["q_rl"], s["t_rl"], [0] * 5, s["cams"], k, n_left)
    p = msorb_mod.pose_rig_problem(s["q"], s["t"], s["cams"], s["q_rl"], s["t_rl"], n_points)
    res, out = msorb_mod.pose_optimization_rig_batch(p, s["xy"], s["camera"], s["inv_sigma2"], s["pos_w"])
    r = res[0]
    stale = np.arange(n_keys) % 3 == 0
    want_flags = stale.copy()
    want_flags[k["slots"]] = out                            # entries without a usable point keep their flags
    if n_points >= 3:
        assert 0 < r["n_bad"] < n_points and r["iterations"].min() > 0
        if len(cams) == 2:
            assert 0 < s["camera"].sum() < n_points         # matched points in both cameras
        assert n_set == 1 and ret == int(r["n_initial"] - r["n_bad"])
        assert np.array_equal(pose.view(np.uint32), np.concatenate([r["q"], r["t"]]).view(np.uint32))
    else:                                                   # :936-937: 0 returned, the pose left alone, the flags cleared
        assert ret == 0 and n_set == 0 and np.array_equal(pose, np.concatenate([s["q"], s["t"]])) and not out.any()
    assert np.array_equal(flags, want_flags)
    assert (k["state"] == 2).sum() > 5 and np.array_equal(flags[k["state"] != 1], stale[k["state"] != 1])


def test_a_pinhole_frame_takes_the_old_path(exe, tmp_path, msorb_mod):
    n_points, n_keys = 400, 1000
    s = pc.make_scene(54, n_points, stereo=0.6, outliers=0.2, rot_deg=1.5, trans=0.15)
    k, inv, n_left = _frame(54, s["xy"], np.zeros(n_points, np.uint8), s["pos_w"], n_keys, False)
    k["ur"][k["slots"]] = s["u_right"]
    s["inv_sigma2"] = inv
    c = s["cam"]
    pin = [c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"]]
    any_camera, old = _run(exe, tmp_path, s["q"], s["t"], None, None, pin, [(rc.PINHOLE, pin[:4])], k, n_left)
    res, out = msorb_mod.pose_optimization_batch(msorb_mod.pose_problem(s["q"], s["t"], c, n_points), s["xy"], s["u_right"], s["inv_sigma2"],
                                                 s["pos_w"])
    r = res[0]
    assert (s["u_right"] >= 0).sum() > 100 and 0 < r["n_bad"] < n_points          # stereo edges: only the old entry has them
    for ret, n_set, pose, flags in (any_camera, old):
        assert ret == int(r["n_initial"] - r["n_bad"]) and n_set == 1
        assert np.array_equal(pose.view(np.uint32), np.concatenate([r["q"], r["t"]]).view(np.uint32))
        assert np.array_equal(flags[k["slots"]], out)
    assert np.array_equal(any_camera[3], old[3])


@pytest.mark.parametrize("what", ["unknown_type", "stereo_observation_on_a_fisheye_frame"])
def test_refusals_leave_the_frame_alone(exe, tmp_path, what):
    cams = ("kb8", "kb8") if what == "unknown_type" else ("kb8",)
    s, k, n_left = _rig_case(55, 100, 300, cams)
    cam_list = list(s["cams"])
    if what == "unknown_type":
        cam_list[1] = (7, cam_list[1][1])
    else:
        k["ur"][k["slots"][40]] = 123.0
    (ret, n_set, pose, flags), = _run(exe, tmp_path, s["q"], s["t"], s["q_rl"], s["t_rl"], [0] * 5, cam_list, k, n_left)
    assert ret == -1 and n_set == 0
    assert np.array_equal(pose, np.concatenate([s["q"], s["t"]])) and np.array_equal(flags, np.arange(300) % 3 == 0)
