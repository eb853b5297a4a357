"""Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame on the device (csrc/pose_inertial.hip) through the C ABI and its
Python mirror, against the forward restatement of tests/pose_inertial_cases.py and against the host program (the same header
through g++ and glibc).

Bounds: those of tests/test_pose_inertial_cpu.py.  D is the largest difference between the forward restatement and any of its
variants over these very scenes (tests/golden/pose_inertial_sensitivity.json); the device adds in one more order and has another
libm, so it may differ by 16 D (DESIGN.md sections 9 to 20).  Flags, counts and round lengths are equal: the CPU test shows that no
compared chi2 comes within 100 times the chi2 spread of a threshold.  Byte-equality with the host program is printed, not required.
The per-edge chi2 is NOT compared for the device: the C ABI does not return it.  It is checked there only through the flags and
counts it decides; tests/test_pose_inertial_cpu.py compares it for the host program, which compiles the kernel's text."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from msorb import synth
import pose_inertial_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = tuple(pc.GPU_SCENES) + tuple("chain3/%d" % i for i in range(3))
MBF = float(np.float32(pc.KITTI["mbf"]))
MB = MBF / pc.KITTI["fx"]
BOUNDS = (0.0, 1241.0, 0.0, 376.0)


def _scene(name):
    return pc.chain3()[int(name[-1])] if name.startswith("chain3") else pc.scene(name)


def _run(msorb_mod, scenes):
    return msorb_mod.pose_inertial_optimization_batch(*pc.flat(scenes))


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_inertial_gpu")
    exe = str(d / "pose_inertial_main")
    b = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", os.path.join(ROOT, "tests", "pose_inertial_main.cc"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    scenes = [_scene(n) for n in ALL]
    pc.write_scenes(str(d / "in.bin"), scenes)
    p = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-2000:])
    return dict(zip(ALL, pc.read_results(str(d / "out.bin"), scenes)))


def test_capacity_is_what_the_scenes_assume(msorb_mod):
    assert msorb_mod.pose_inertial_optimization_capacity() == pc.CAPACITY
    assert msorb_mod.POSE_INERTIAL_PROBLEM_DTYPE == pc.PROBLEM_DTYPE and msorb_mod.POSE_INERTIAL_RESULT_DTYPE == pc.RESULT_DTYPE


def _compare(name, sc, r, other, what):
    g, b = pc.golden(), pc.bounds()
    d = pc.differences(other, r, sc)
    print(f"{name}: device / {what}: {pc.decisions(r)[1:]} / {pc.decisions(other)[1:]}, in D: "
          + " ".join(f"{q} {d[q] / g['D'][q]:.4f}" for q in d))
    assert pc.decisions(r) == pc.decisions(other), (name, what)
    assert pc.within(d, b), (name, what, d, b)


@pytest.mark.parametrize("name", ALL)
def test_against_the_restatement(msorb_mod, host_results, name):
    sc = _scene(name)
    form = int(sc["problem"]["form"])
    res, out = _run(msorb_mod, [sc])
    again, out2 = _run(msorb_mod, [sc])
    r = pc.as_result(res[0], out, form=form)
    _compare(name, sc, r, pc.optimize(sc), "restatement")
    rec, h = host_results[name]
    _compare(name, sc, r, h, "host program")
    print(f"{name}: byte-equal to the host program: {res[0].tobytes() == rec.tobytes() and np.array_equal(out, h['flags'])}")
    assert res.tobytes() == again.tobytes() and np.array_equal(out, out2)             # a second run returns the same bits
    assert int(res[0]["n_initial"]) == int(sc["problem"]["n"])
    assert np.array_equal(res[0]["Rwb_f"], res[0]["est"]["Rwb"].astype(np.float32))  # what SetImuPoseVelocity receives
    assert np.array_equal(res[0]["twb_f"], res[0]["est"]["twb"].astype(np.float32))
    assert np.array_equal(res[0]["v_f"], res[0]["est"]["v"].astype(np.float32))
    assert np.isfinite(res[0]["H_raw"]).all() and np.isfinite(res[0]["H_prior"]).all()


def test_a_batch_equals_the_single_calls(msorb_mod):
    names = ("n0/1", "n257/0", "mixed/1", "n6/0", "n6/1", "close_points/0", "huber_prior/1", "solver_fails/0")
    scenes = [_scene(n) for n in names]
    res, out = _run(msorb_mod, scenes)
    k = 0
    for i, sc in enumerate(scenes):
        one, flags = _run(msorb_mod, [sc])
        n = int(sc["problem"]["n"])
        assert one[0].tobytes() == res[i].tobytes() and np.array_equal(flags, out[k:k + n]), names[i]
        k += n
    # one problem above the register capacity in a batch with one below: both stores in one launch
    scenes = [_scene("capacity_plus_1/0"), _scene("n255/1")]
    res, out = _run(msorb_mod, scenes)
    for i, sc in enumerate(scenes):
        one, flags = _run(msorb_mod, [sc])
        lo = 0 if i == 0 else pc.CAPACITY + 1
        assert one[0].tobytes() == res[i].tobytes() and np.array_equal(flags, out[lo:lo + int(sc["problem"]["n"])])


@pytest.fixture(scope="module")
def kitti_frame(msorb_mod):
    """keypoints, mvuRight and octaves of an extracted synthetic stereo pair"""
    cfg = synth.KITTI
    L, R = synth.stereo_pair(21, cfg["rows"], cfg["cols"])
    ex = msorb_mod.ORBextractor(2000, 1.2, 8, 20, 7)
    kl, dl, kr, dr, ur, dp, oob = ex.extract_stereo(L, R, MB, MBF)
    scale = np.asarray(ex.GetScaleFactors(), np.float32)
    ex.close()
    inv_level = (1.0 / (scale.astype(np.float64) ** 2)).astype(np.float32)
    return dict(kl=kl, dl=dl, ur=np.asarray(ur, np.float32), scale=scale, inv_level=inv_level)


def _frame_case(fr, seed, form):
    """-> problem, has_point, pos_w [N, 3], close [N]: the inertial part of a generated scene, map points that fit the frame's
    keypoints under that scene's true camera pose, 60 % of the keypoints with a point, 10 % of those wrong"""
    sc = pc.build(seed, 0, form)
    rng = np.random.default_rng(seed)
    t = sc["truth"]
    Rcw = pc.RCB @ t["Rwb"].T
    tcw = pc.RCB @ (-t["Rwb"].T @ t["twb"]) + pc.TCB
    n = len(fr["kl"])
    x, y, ur = fr["kl"]["x"].astype(np.float64), fr["kl"]["y"].astype(np.float64), fr["ur"].astype(np.float64)
    z = np.where(ur >= 0, MBF / np.maximum(x - ur, 0.5), rng.uniform(4, 40, n))
    sig = fr["scale"][fr["kl"]["octave"]].astype(np.float64)
    xn, yn = x + 0.6 * rng.normal(size=n) * sig, y + 0.6 * rng.normal(size=n) * sig
    wrong = rng.uniform(size=n) < 0.1
    xn[wrong] += rng.uniform(20, 200, n)[wrong] * rng.choice([-1, 1], n)[wrong]
    Xc = np.stack([(xn - pc.KITTI["cx"]) / pc.KITTI["fx"] * z, (yn - pc.KITTI["cy"]) / pc.KITTI["fy"] * z, z], -1)
    Xw = (Xc - tcw[None]) @ Rcw
    has = (rng.uniform(size=n) < 0.6).astype(np.uint8)
    return sc["problem"], has, Xw.astype(np.float32), (z < 10.0).astype(np.uint8)


def _flat_of_frame(msorb_mod, fr, p, has, Xw, close):
    m = has.astype(bool)
    p = p.copy()
    p["n"] = int(m.sum())
    xy = np.stack([fr["kl"]["x"][m], fr["kl"]["y"][m]], -1)
    res, out = msorb_mod.pose_inertial_optimization_batch(p, xy, fr["ur"][m], fr["inv_level"][fr["kl"]["octave"][m]], Xw[m], close[m])
    return res[0], out


@pytest.mark.parametrize("form", (0, 1))
def test_frame_form_equals_flat_form(msorb_mod, kitti_frame, form):
    fr = kitti_frame
    assert len(fr["kl"]) > 1500 and (fr["ur"] >= 0).sum() > 300 and (fr["ur"] < 0).sum() > 300
    f = msorb_mod.Frame(fr["kl"], fr["dl"], fr["ur"], BOUNDS, fr["scale"])
    p, has, Xw, close = _frame_case(fr, 50 + form, form)
    before = (np.arange(len(has)) % 2).astype(np.uint8)
    r, out = f.pose_inertial_optimization(p, has, Xw, close, fr["inv_level"], outlier=before.copy())
    r_flat, out_flat = _flat_of_frame(msorb_mod, fr, p, has, Xw, close)
    m = has.astype(bool)
    print("frame form:", int(r["n_initial"]), int(r["n_bad"]), int(r["n_inliers"]), r["iterations"].tolist())
    assert r.tobytes() == r_flat.tobytes()
    assert np.array_equal(out[m].astype(bool), out_flat)
    assert np.array_equal(out[~m], before[~m])               # left alone where there is no point
    assert r["n_initial"] == m.sum() and 0 < r["n_bad"] < 0.4 * m.sum() and r["iterations"].min() == 10
    for field, value in (("form", 3), ("mbf", np.nan)):          # the frame entry refuses what the flat one refuses
        bad = p.copy()
        bad[field] = value
        untouched = before.copy()
        with pytest.raises(msorb_mod.MsorbError) as e:
            f.pose_inertial_optimization(bad, has, Xw, close, fr["inv_level"], outlier=untouched)
        assert e.value.code == msorb_mod.E_INVALID and "frame_pose_inertial_optimization:" in str(e.value)
        assert np.array_equal(untouched, before)
    f.close()


def test_frame_form_from_three_threads(msorb_mod, kitti_frame):
    fr = kitti_frame
    cases = [_frame_case(fr, 60 + k, k % 2) for k in range(3)]
    want = [_flat_of_frame(msorb_mod, fr, *c) for c in cases]
    frames = [msorb_mod.Frame(fr["kl"], fr["dl"], fr["ur"], BOUNDS, fr["scale"]) for _ in range(3)]
    got, errors = [None] * 3, []

    def work(k):
        try:
            for _ in range(3):
                p, has, Xw, close = cases[k]
                got[k] = frames[k].pose_inertial_optimization(p, has, Xw, close, fr["inv_level"])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(3)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for k in range(3):
        m = cases[k][1].astype(bool)
        assert got[k][0].tobytes() == want[k][0].tobytes() and np.array_equal(got[k][1][m].astype(bool), want[k][1]), k
    for f in frames:
        f.close()


def test_refusals_leave_the_device_usable(msorb_mod):
    sc = _scene("mixed/1")
    pr, xy, ur, inv, pos, close = pc.flat([sc])
    INV = msorb_mod.E_INVALID

    def refused(pr=pr, xy=xy, ur=ur, inv=inv, pos=pos, close=close):
        with pytest.raises(msorb_mod.MsorbError) as e:
            msorb_mod.pose_inertial_optimization_batch(pr, xy, ur, inv, pos, close)
        assert e.value.code == INV and "pose_inertial_optimization_batch:" in str(e.value)     # msorb_last_error()'s text

    for field, value in (("form", 2), ("form", -1)):
        bad = pr.copy()
        bad[field] = value
        refused(pr=bad)
    for field in ("Rcw", "tbc", "info_gyro", "H"):
        bad = pr.copy()
        bad[field][0, 1] = np.nan
        refused(pr=bad)
    for group, field in (("frame", "twb"), ("other", "bg"), ("prior", "Rwb"), ("pre", "dV"), ("pre", "info")):
        bad = pr.copy()
        bad[group][field][0, 0] = np.inf
        refused(pr=bad)
    bad = pr.copy()
    bad["mbf"] = np.nan
    refused(pr=bad)
    for k, a in (("xy", xy), ("ur", ur), ("inv", inv), ("pos", pos)):
        b = a.copy()
        b.reshape(-1)[3] = np.nan
        refused(**{k: b})
    L = msorb_mod.lib()
    vp, ci = C.c_void_p, C.c_int
    L.msorb_pose_inertial_optimization_batch.argtypes = [ci, ci] + [vp] * 10
    n = int(pr["n"][0])
    off = np.array([0, n], np.int32)
    out, res = np.full(n, 7, np.uint8), np.zeros(1, pc.RESULT_DTYPE)
    res["n_bad"] = -7
    p = lambda a: a.ctypes.data  # noqa: E731
    good = [0, 1, p(pr), p(off), p(xy), p(ur), p(inv), p(pos), p(close), p(out), p(res), None]
    for i in (2, 3, 4, 5, 6, 7, 8, 9, 10):                                                        # null pointers
        args = list(good)
        args[i] = None
        assert L.msorb_pose_inertial_optimization_batch(*args) == INV, i
    args = list(good)
    args[1] = -1                                                                                  # a negative count
    assert L.msorb_pose_inertial_optimization_batch(*args) == INV
    for bad_off in ((1, n + 1), (0, n - 1)):                                                      # inconsistent offsets
        args = list(good)
        o = np.array(bad_off, np.int32)
        args[3] = p(o)
        assert L.msorb_pose_inertial_optimization_batch(*args) == INV
    assert (out == 7).all() and int(res["n_bad"][0]) == -7                                        # no output written
    # one valid call afterwards passes
    r, flags = _run(msorb_mod, [sc])
    _compare("mixed/1", sc, pc.as_result(r[0], flags, form=1), pc.optimize(sc), "restatement after the refusals")
