"""ms-slam_amd/host/Optimizer_device.h compiled against stand-in Frame / MapPoint / Pinhole types (tests/dropin_poseopt_main.cc),
linked to libmsorb.so through the C ABI and run on the GPU: mvbOutlier, the pose SetPose received and the return value equal
what the Python mirror computes for the same seed, in the flat form and with the keypoints resident on a handle; a frame with a
second camera comes back untouched with -1."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.dirname(os.path.abspath(__file__))]
import pose_opt_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("poseopt") / "dropin_poseopt"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include",
                           f"{ROOT}/tests/dropin_poseopt_main.cc", f"-L{ROOT}/ms-slam_amd", "-lmsorb", f"-Wl,-rpath,{ROOT}/ms-slam_amd",
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", str(out)])
    return out


def _frame_of_scene(seed, n_points, n_keys, n_levels=8):
    """A frame of n_keys keypoints of which n_points (spread over the frame) carry the observations of a scene; every 7th of the
    other keypoints carries a bad map point, the rest none.  -> the scene, per-keypoint arrays, the level table"""
    s = pc.make_scene(seed, n_points, stereo=0.6, outliers=0.2, rot_deg=1.5, trans=0.15)
    rng = np.random.default_rng(seed + 1000)
    slots = np.sort(rng.choice(n_keys, n_points, replace=False))
    inv_level = (1.0 / (1.2 ** np.arange(n_levels)) ** 2).astype(np.float32)
    octave = rng.integers(0, n_levels, n_keys).astype(np.int32)
    s["inv_sigma2"] = inv_level[octave[slots]]          # the scene's weights become the frame's level table
    x = rng.uniform(0, 1241, n_keys).astype(np.float32)
    y = rng.uniform(0, 376, n_keys).astype(np.float32)
    ur = np.where(rng.uniform(size=n_keys) < 0.5, x - 20, -1).astype(np.float32)
    pos = rng.uniform(-10, 10, (n_keys, 3)).astype(np.float32)
    state = np.where(np.arange(n_keys) % 7 == 0, 2, 0).astype(np.int32)
    x[slots], y[slots], ur[slots], pos[slots], state[slots] = s["xy"][:, 0], s["xy"][:, 1], s["u_right"], s["pos_w"], 1
    return s, dict(x=x, y=y, ur=ur, octave=octave, state=state, pos=pos, slots=slots), inv_level


def _write(path, s, k, inv_level):
    c = s["cam"]
    with open(path, "wb") as f:
        f.write(np.concatenate([s["q"], s["t"], np.array([c["fx"], c["fy"], c["cx"], c["cy"], c["mbf"]], np.float32)]).astype("<f4").tobytes())
        f.write(struct.pack("<ii", len(k["x"]), len(inv_level)))
        f.write(inv_level.astype("<f4").tobytes())
        for i in range(len(k["x"])):
            f.write(struct.pack("<fffiifff", k["x"][i], k["y"][i], k["ur"][i], k["octave"][i], k["state"][i], *k["pos"][i]))


def _read(blob, n_keys):
    runs, pos = [], 0
    for _ in range(3):
        ret, = struct.unpack_from("<i", blob, pos)
        pose = np.frombuffer(blob, "<f4", 7, pos + 4)
        flags = np.frombuffer(blob, np.uint8, n_keys, pos + 32).astype(bool)
        runs.append((ret, pose, flags))
        pos += 32 + n_keys
    assert pos == len(blob)
    return runs


@pytest.mark.parametrize("seed,n_points,n_keys", [(41, 700, 1900), (42, 2, 50)])
def test_host_template(exe, tmp_path, msorb_mod, seed, n_points, n_keys):
    s, k, inv_level = _frame_of_scene(seed, n_points, n_keys)
    _write(tmp_path / "in.bin", s, k, inv_level)
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    flat, resident, rig = _read((tmp_path / "out.bin").read_bytes(), n_keys)
    p = msorb_mod.pose_problem(s["q"], s["t"], s["cam"], n_points)
    res, out = msorb_mod.pose_optimization_batch(p, s["xy"], s["u_right"], s["inv_sigma2"], s["pos_w"])
    r = res[0]
    stale = np.arange(n_keys) % 3 == 0
    want_flags = stale.copy()
    want_flags[k["slots"]] = out                       # n < 3: cleared (:810, :837)
    want_pose = np.concatenate([r["q"], r["t"]])
    want_ret = int(r["n_initial"] - r["n_bad"])
    if n_points >= 3:
        assert 0 < r["n_bad"] < n_points and r["iterations"].min() > 0
    else:
        assert want_ret == 0 and np.array_equal(want_pose, np.concatenate([s["q"], s["t"]]))
    for name, (ret, pose, flags) in (("flat", flat), ("resident", resident)):
        assert ret == want_ret, name
        assert np.array_equal(pose.view(np.uint32), want_pose.view(np.uint32)), name
        assert np.array_equal(flags, want_flags), name
    ret, pose, flags = rig                             # mpCamera2: -1, nothing touched
    assert ret == -1
    assert np.array_equal(pose, np.concatenate([s["q"], s["t"]])) and np.array_equal(flags, stale)
