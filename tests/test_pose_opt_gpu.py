"""Optimizer::PoseOptimization on the device (csrc/pose_opt.hip) through the C ABI against the float64 restatement of
tests/pose_opt_cases.py ('forward' order = g2o's walk over its edge list).

Bounds.  D is the largest difference the restatement's three summation orders make on the pose over these very scenes (committed in
tests/golden/pose_opt_sensitivity.json, re-checked by tests/test_pose_opt_cpu.py); the kernel adds in a fourth order (thread,
wavefront butterfly, wavefronts), so its double pose may differ from the restatement's by 16 D.  Flags and counts must be equal:
tests/test_pose_opt_cpu.py::test_threshold_margin shows no chi2 comes close enough to a threshold for an order to matter."""
import json
import threading

import numpy as np
import pytest

from msorb import synth
import pose_opt_cases as pc

pytestmark = pytest.mark.gpu

FIELDS = ("q", "t", "qd", "td", "n_initial", "n_bad", "iterations", "rejected_trials")


@pytest.fixture(scope="module")
def golden():
    with open(pc.GOLDEN) as f:
        return json.load(f)


def _run(msorb_mod, s):
    n = len(s["u_right"])
    p = msorb_mod.pose_problem(s["q"], s["t"], s["cam"], n)
    res, out = msorb_mod.pose_optimization_batch(p, s["xy"], s["u_right"], s["inv_sigma2"], s["pos_w"])
    return res[0], out


def _same(a, b):
    return all(np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes() for f in FIELDS)


def _float_close(a, b):
    """1 float ulp per component; components below 1e-6 in magnitude: 1e-7 absolute"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    big = np.maximum(np.abs(a), np.abs(b))
    tol = np.where(big < 1e-6, np.float32(1e-7), np.spacing(big))
    return bool(np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= tol.astype(np.float64)))


def test_capacity_is_what_the_scenes_assume(msorb_mod):
    assert msorb_mod.pose_optimization_capacity() == pc.CAPACITY and pc.CAPACITY % pc.WORKGROUP == 0


@pytest.mark.parametrize("name", list(pc.GPU_SCENES))
def test_against_the_restatement(msorb_mod, golden, name):
    s, ref = pc.scene(name), pc.reference(name)
    r, out = _run(msorb_mod, s)
    bound = golden["pose_bound"]
    agree = pc.orders_agree(name)
    if ref["n_initial"] >= 3:
        dq = float(np.max(np.abs(pc.sign_aligned(r["qd"], ref["qd"]) - ref["qd"])))
        dt = float(np.max(np.abs(r["td"] - ref["td"]))) / s["median_depth"]
    else:
        dq = dt = 0.0
    print(f"{name}: dq={dq:.3e} dt/depth={dt:.3e} bound={bound:.3e} it={r['iterations'].tolist()} ref={ref['iterations']} "
          f"rej={r['rejected_trials'].tolist()} ref={ref['rejected_trials']} orders_agree={agree} "
          f"n_bad={int(r['n_bad'])} ref={ref['n_bad']} flags_differ={int(np.sum(out != ref['outlier']))}")
    # outliers and counts: equal
    assert np.array_equal(out, ref["outlier"])
    assert r["n_initial"] == ref["n_initial"] and r["n_bad"] == ref["n_bad"]
    # the float pose is the narrowing of the device's own double
    if ref["n_initial"] >= 3:
        assert np.array_equal(r["q"], r["qd"].astype(np.float32)) and np.array_equal(r["t"], r["td"].astype(np.float32))
    else:   # :936-937: untouched
        assert np.array_equal(r["q"], s["q"]) and np.array_equal(r["t"], s["t"])
    # pose
    assert dq <= bound and dt <= bound
    sign = -1.0 if np.dot(r["qd"], ref["qd"]) < 0 else 1.0
    assert _float_close(sign * r["q"], ref["q"]) and _float_close(r["t"], ref["t"])
    # iterations, where the CPU orders agree among themselves
    if agree:
        assert r["iterations"].tolist() == ref["iterations"] and r["rejected_trials"].tolist() == ref["rejected_trials"]
    else:
        assert [int(v) >= 0 for v in r["iterations"]] == [v >= 0 for v in ref["iterations"]]
    if name == "rejected_trials":
        assert sum(ref["rejected_trials"]) > 0       # the stale-error rule is exercised
    if name == "all_outliers":
        assert r["iterations"].tolist()[1:] == [0, 0, 0] and r["n_bad"] == r["n_initial"]


def _batch_inputs(msorb_mod, names):
    ss = [pc.scene(n) for n in names]
    probs = np.concatenate([msorb_mod.pose_problem(s["q"], s["t"], s["cam"], len(s["u_right"])) for s in ss])
    cat = lambda k: np.concatenate([np.asarray(s[k]).reshape(len(s["u_right"]), -1) for s in ss]).astype(np.float32)   # noqa: E731
    return ss, probs, cat("xy"), cat("u_right").reshape(-1), cat("inv_sigma2").reshape(-1), cat("pos_w")


def test_batch_equals_single_calls(msorb_mod):
    ss, probs, xy, ur, inv, pos = _batch_inputs(msorb_mod, pc.BATCH_SCENES)
    assert len(ss) == 8
    res, out = msorb_mod.pose_optimization_batch(probs, xy, ur, inv, pos)
    o = 0
    for k, s in enumerate(ss):
        r1, out1 = _run(msorb_mod, s)
        n = len(s["u_right"])
        assert _same(res[k], r1), pc.BATCH_SCENES[k]
        assert np.array_equal(out[o:o + n], out1), pc.BATCH_SCENES[k]
        o += n


def test_a_batch_with_resident_and_strided_problems(msorb_mod):
    names = ("n2", "capacity_plus_1", "n64")
    ss, probs, xy, ur, inv, pos = _batch_inputs(msorb_mod, names)
    res, out = msorb_mod.pose_optimization_batch(probs, xy, ur, inv, pos)
    o = 0
    for k, s in enumerate(ss):
        r1, out1 = _run(msorb_mod, s)
        n = len(s["u_right"])
        assert _same(res[k], r1) and np.array_equal(out[o:o + n], out1), names[k]
        o += n


@pytest.mark.parametrize("name", ["mixed", "n5000"])
def test_two_runs_are_bit_identical(msorb_mod, name):
    s = pc.scene(name)
    a, oa = _run(msorb_mod, s)
    b, ob = _run(msorb_mod, s)
    assert _same(a, b) and np.array_equal(oa, ob)


# ---------------------------------------------------------------------------------------------------------- frame form
MBF = pc.KITTI["mbf"]
MB = MBF / pc.KITTI["fx"]
BOUNDS = (0.0, 1241.0, 0.0, 376.0)


@pytest.fixture(scope="module")
def kitti_frame(msorb_mod):
    """keypoints, mvuRight and octaves of an extracted synthetic stereo pair, and map points that fit them"""
    cfg = synth.KITTI
    L, R = synth.stereo_pair(21, cfg["rows"], cfg["cols"])
    ex = msorb_mod.ORBextractor(2000, 1.2, 8, 20, 7)
    kl, dl, kr, dr, ur, dp, oob = ex.extract_stereo(L, R, MB, MBF)
    scale = np.asarray(ex.GetScaleFactors(), np.float32)
    ex.close()
    inv_level = (1.0 / (scale.astype(np.float64) ** 2)).astype(np.float32)
    return dict(kl=kl, dl=dl, ur=np.asarray(ur, np.float32), scale=scale, inv_level=inv_level)


def _frame_case(fr, seed):
    """-> q, t, has_point, pos_w [N, 3]: a pose near the identity, 60 % of the keypoints with a point, 15 % of those wrong"""
    rng = np.random.default_rng(seed)
    n = len(fr["kl"])
    cam = {k: float(np.float32(v)) for k, v in pc.KITTI.items()}
    x, y, ur = fr["kl"]["x"].astype(np.float64), fr["kl"]["y"].astype(np.float64), fr["ur"].astype(np.float64)
    z = np.where(ur >= 0, cam["mbf"] / np.maximum(x - ur, 0.5), rng.uniform(4, 40, n))
    sig = fr["scale"][fr["kl"]["octave"]].astype(np.float64)
    xn, yn = x + rng.normal(size=n) * sig, y + rng.normal(size=n) * sig
    wrong = rng.uniform(size=n) < 0.15
    xn[wrong] += rng.uniform(20, 200, n)[wrong] * rng.choice([-1, 1], n)[wrong]
    Xc = np.stack([(xn - cam["cx"]) / cam["fx"] * z, (yn - cam["cy"]) / cam["fy"] * z, z], -1)
    q_true = pc._quat_from_axis_angle(rng.normal(size=3), np.radians(3.0))
    t_true = rng.uniform(-1, 1, 3)
    Xw = pc.rotate(q_true * np.array([-1, -1, -1, 1.0]), Xc - t_true)
    dq = pc._quat_from_axis_angle(rng.normal(size=3), np.radians(1.0))
    q0 = pc._quat_mul(dq, q_true)
    t0 = pc.rotate(dq, t_true) + rng.normal(size=3) * 0.05
    has = (rng.uniform(size=n) < 0.6).astype(np.uint8)
    return cam, q0.astype(np.float32), t0.astype(np.float32), has, Xw.astype(np.float32)


def _flat_of_frame(msorb_mod, fr, cam, q, t, has, Xw):
    m = has.astype(bool)
    xy = np.stack([fr["kl"]["x"][m], fr["kl"]["y"][m]], -1)
    p = msorb_mod.pose_problem(q, t, cam, int(m.sum()))
    res, out = msorb_mod.pose_optimization_batch(p, xy, fr["ur"][m], fr["inv_level"][fr["kl"]["octave"][m]], Xw[m])
    return res[0], out


def test_frame_form_equals_flat_form(msorb_mod, kitti_frame):
    fr = kitti_frame
    assert len(fr["kl"]) > 1500 and (fr["ur"] >= 0).sum() > 300 and (fr["ur"] < 0).sum() > 300
    f = msorb_mod.Frame(fr["kl"], fr["dl"], fr["ur"], BOUNDS, fr["scale"])
    cam, q, t, has, Xw = _frame_case(fr, 5)
    stale = (np.arange(len(has)) % 2).astype(np.uint8)
    r, out = f.pose_optimization(q, t, cam, has, Xw, fr["inv_level"], outlier=stale.copy())
    r_flat, out_flat = _flat_of_frame(msorb_mod, fr, cam, q, t, has, Xw)
    m = has.astype(bool)
    print("frame form:", int(r["n_initial"]), int(r["n_bad"]), r["iterations"].tolist(), r["rejected_trials"].tolist())
    assert _same(r, r_flat)
    assert np.array_equal(out[m].astype(bool), out_flat)
    assert np.array_equal(out[~m], stale[~m])            # left alone where there is no point
    assert r["n_initial"] == m.sum() and 0 < r["n_bad"] < 0.4 * m.sum() and r["iterations"].min() > 0
    f.close()


def test_frame_form_from_three_threads(msorb_mod, kitti_frame):
    fr = kitti_frame
    cases = [_frame_case(fr, 11 + k) for k in range(3)]
    want = [_flat_of_frame(msorb_mod, fr, *c) for c in cases]
    frames = [msorb_mod.Frame(fr["kl"], fr["dl"], fr["ur"], BOUNDS, fr["scale"]) for _ in range(3)]
    got, errors = [None] * 3, []

    def work(k):
        try:
            for _ in range(4):
                cam, q, t, has, Xw = cases[k]
                got[k] = frames[k].pose_optimization(q, t, cam, has, Xw, fr["inv_level"])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(3)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for k in range(3):
        m = cases[k][3].astype(bool)
        assert _same(got[k][0], want[k][0]) and np.array_equal(got[k][1][m].astype(bool), want[k][1]), k
    for f in frames:
        f.close()
