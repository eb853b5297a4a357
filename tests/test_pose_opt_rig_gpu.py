"""Optimizer::PoseOptimization of a two-camera / non-pinhole frame on the device (msorb_pose_optimization_rig_batch, the RigModel of
csrc/pose_opt.hip over csrc/pose_rig_device.h) through the C ABI against the float64 restatement of tests/pose_opt_rig_cases.py
('forward' order, unperturbed).

Bounds.  D is the largest difference the restatement's variants (three summation orders; theta / psi of project one float ulp up or
down; the double atan2 / sin / cos / sqrt one ulp up or down) make on the pose over these very scenes, committed in
tests/golden/pose_opt_rig_sensitivity.json and re-checked by tests/test_pose_opt_rig_cpu.py; the kernel adds in a fourth order and
takes atan2f as a narrowed double atan2, so its double pose may differ from the restatement's by 16 D.  Flags and counts must be
equal: tests/test_pose_opt_rig_cpu.py::test_threshold_margin shows no chi2 comes within 16 C of its threshold under any variant."""
import json
import os
import subprocess

import numpy as np
import pytest

import pose_opt_cases as pc
import pose_opt_rig_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("q", "t", "qd", "td", "n_initial", "n_bad", "iterations", "rejected_trials")


@pytest.fixture(scope="module")
def golden():
    with open(rc.GOLDEN) as f:
        return json.load(f)


def _problem(msorb_mod, s):
    return msorb_mod.pose_rig_problem(s["q"], s["t"], s["cams"], s["q_rl"], s["t_rl"], len(s["camera"]))


def _run(msorb_mod, s):
    res, out = msorb_mod.pose_optimization_rig_batch(_problem(msorb_mod, s), s["xy"], s["camera"], s["inv_sigma2"], s["pos_w"])
    return res[0], out


def _same(a, b):
    return all(np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes() for f in FIELDS)


def _distance(r, ref, s):
    """-> the largest component difference of qd (sign-aligned) and of td / median depth"""
    if ref["n_initial"] < 3:
        return 0.0, 0.0
    return (float(np.max(np.abs(pc.sign_aligned(r["qd"], ref["qd"]) - ref["qd"]))),
            float(np.max(np.abs(r["td"] - ref["td"]))) / s["median_depth"])


def test_capacity_is_what_the_scenes_assume(msorb_mod):
    assert msorb_mod.pose_optimization_rig_capacity() == rc.CAPACITY and rc.CAPACITY % rc.WORKGROUP == 0


def test_the_scenes_reach_what_they_are_named_for():
    s = rc.scene("rig")
    assert 0.4 < s["camera"].mean() < 0.6 and np.all(np.diff(s["camera"].astype(int)) >= 0)                # half and half, sorted
    si = rc.scene("rig_interleaved")
    assert np.array_equal(np.sort(si["camera"]), s["camera"]) and np.sum(np.diff(si["camera"].astype(int)) != 0) > 300
    assert rc.scene("right_only")["camera"].all() and not rc.scene("fisheye_mono")["camera"].any()
    assert rc.scene("fisheye_mono")["n_cameras"] == 1
    w = rc.scene("wide")
    E = rc.RigEdges(w["cams"], w["q_rl"], w["t_rl"], w["xy"], w["camera"], w["inv_sigma2"], w["pos_w"])
    ref = rc.reference("wide")
    _, Xl, _ = E.error(list(ref["qd"]), list(ref["td"]))
    assert np.sum((Xl[:, 2] < 0) & ~ref["outlier"] & (w["camera"] == 0)) >= 3                               # inliers with z < 0
    assert sum(rc.reference("rejected_trials")["rejected_trials"]) > 0


@pytest.mark.parametrize("name", list(rc.GPU_SCENES))
def test_against_the_restatement(msorb_mod, golden, name):
    s, ref = rc.scene(name), rc.reference(name)
    r, out = _run(msorb_mod, s)
    bound = golden["pose_bound"]
    agree = rc.variants_agree(name)
    dq, dt = _distance(r, ref, s)
    print(f"{name}: dq={dq:.3e} dt/depth={dt:.3e} bound={bound:.3e} it={r['iterations'].tolist()} ref={ref['iterations']} "
          f"rej={r['rejected_trials'].tolist()} ref={ref['rejected_trials']} variants_agree={agree} "
          f"n_bad={int(r['n_bad'])} ref={ref['n_bad']} flags_differ={int(np.sum(out != ref['outlier']))}")
    assert np.array_equal(out, ref["outlier"])
    assert r["n_initial"] == ref["n_initial"] and r["n_bad"] == ref["n_bad"]
    if ref["n_initial"] >= 3:      # the float pose is the narrowing of the device's own double
        assert np.array_equal(r["q"], r["qd"].astype(np.float32)) and np.array_equal(r["t"], r["td"].astype(np.float32))
    else:                          # :936-937: untouched
        assert np.array_equal(r["q"], s["q"]) and np.array_equal(r["t"], s["t"])
        assert r["iterations"].tolist() == [-1] * 4 and not out.any()
    assert dq <= bound and dt <= bound
    if agree:
        assert r["iterations"].tolist() == ref["iterations"] and r["rejected_trials"].tolist() == ref["rejected_trials"]
    else:
        assert [int(v) >= 0 for v in r["iterations"]] == [v >= 0 for v in ref["iterations"]]
    if name == "n9":
        assert r["iterations"].tolist()[1:] == [-1, -1, -1] and r["iterations"][0] > 0        # edges().size() < 10: one round
    if name == "n10":
        assert r["iterations"].min() > 0
    if name == "all_outliers":
        assert r["iterations"].tolist()[1:] == [0, 0, 0] and r["n_bad"] == r["n_initial"]


def test_pinhole_equals_the_pinhole_entry(msorb_mod):
    """n_cameras = 1, type 0 on pose_opt_cases' all_mono scene: every field and every flag as msorb_pose_optimization_batch gives
    them with u_right = -1"""
    s = pc.scene("all_mono")
    n = len(s["u_right"])
    assert n == 700 and (s["u_right"] < 0).all()
    c = s["cam"]
    want, want_out = msorb_mod.pose_optimization_batch(msorb_mod.pose_problem(s["q"], s["t"], c, n), s["xy"], s["u_right"], s["inv_sigma2"],
                                                       s["pos_w"])
    p = msorb_mod.pose_rig_problem(s["q"], s["t"], [(rc.PINHOLE, [c["fx"], c["fy"], c["cx"], c["cy"]])], n=n)
    got, got_out = msorb_mod.pose_optimization_rig_batch(p, s["xy"], np.zeros(n, np.uint8), s["inv_sigma2"], s["pos_w"])
    assert want[0]["iterations"].min() > 0 and 0 < want[0]["n_bad"] < n
    assert _same(got[0], want[0]) and np.array_equal(got_out, want_out)


def _batch(msorb_mod, names):
    ss = [rc.scene(n) for n in names]
    probs = np.concatenate([_problem(msorb_mod, s) for s in ss])
    cat = lambda k, dt: np.concatenate([np.asarray(s[k]).reshape(len(s["camera"]), -1) for s in ss]).astype(dt)   # noqa: E731
    return ss, msorb_mod.pose_optimization_rig_batch(probs, cat("xy", np.float32), cat("camera", np.uint8).reshape(-1),
                                                    cat("inv_sigma2", np.float32).reshape(-1), cat("pos_w", np.float32))


def test_batch_equals_single_calls(msorb_mod):
    ss, (res, out) = _batch(msorb_mod, rc.BATCH_SCENES)
    assert len(ss) == 8 and {s["n_cameras"] for s in ss} == {1, 2} and {k for s in ss for k, _ in s["cams"]} == {rc.PINHOLE, rc.KB8}
    assert min(len(s["camera"]) for s in ss) < rc.CAPACITY < max(len(s["camera"]) for s in ss)       # resident and strided
    o = 0
    for k, s in enumerate(ss):
        r1, out1 = _run(msorb_mod, s)
        n = len(s["camera"])
        assert _same(res[k], r1), rc.BATCH_SCENES[k]
        assert np.array_equal(out[o:o + n], out1), rc.BATCH_SCENES[k]
        o += n


@pytest.mark.parametrize("name", ["rig_interleaved", "capacity_plus_1"])
def test_two_runs_are_bit_identical(msorb_mod, name):
    s = rc.scene(name)
    a, oa = _run(msorb_mod, s)
    b, ob = _run(msorb_mod, s)
    assert _same(a, b) and np.array_equal(oa, ob)


def test_invalid_inputs(msorb_mod):
    s = rc.scene("n65")
    good = _problem(msorb_mod, s)

    def refused(p, camera):
        with pytest.raises(msorb_mod.MsorbError) as e:
            msorb_mod.pose_optimization_rig_batch(p, s["xy"], camera, s["inv_sigma2"], s["pos_w"])
        return e.value.code == msorb_mod.E_INVALID

    p = good.copy()
    p["cam"][0, 1]["type"] = 7                       # an unknown camera type
    assert refused(p, s["camera"])
    for k in (0, 3):                                 # n_cameras outside {1, 2}
        p = good.copy()
        p["n_cameras"] = k
        assert refused(p, s["camera"])
    p = good.copy()
    p["n_cameras"] = 1                               # an observation of a right camera the frame does not have
    assert s["camera"].any() and refused(p, s["camera"])
    res, _ = msorb_mod.pose_optimization_rig_batch(p, s["xy"], np.zeros(len(s["camera"]), np.uint8), s["inv_sigma2"], s["pos_w"])
    assert res[0]["n_initial"] == len(s["camera"])   # ... and the same record is accepted without one


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pose_opt_rig_main") / "pose_opt_rig_main"
    b = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "pose_opt_rig_main.cc"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    return str(exe)


@pytest.mark.parametrize("name", ["n65", "fisheye_mono", "rig_interleaved", "wide", "rejected_trials"])
def test_device_against_the_host_program(msorb_mod, golden, host_program, tmp_path, name):
    """the same header run serially on the host (tests/pose_opt_rig_main.cc): flags and counts equal, pose within 16 D"""
    s = rc.scene(name)
    n = len(s["camera"])
    rc.write_problem(tmp_path / "in.bin", s)
    subprocess.run([host_program, "solve", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    h, h_out = rc.read_result(tmp_path / "out.bin", n)
    r, out = _run(msorb_mod, s)
    dq, dt = _distance(r, dict(qd=h["qd"], td=h["td"], n_initial=int(h["n_initial"])), s)
    print(f"{name}: device vs host program dq={dq:.3e} dt/depth={dt:.3e} bound={golden['pose_bound']:.3e} it={r['iterations'].tolist()} "
          f"host={h['iterations'].tolist()} rej={r['rejected_trials'].tolist()} host={h['rejected_trials'].tolist()}")
    assert np.array_equal(out, h_out) and r["n_initial"] == h["n_initial"] and r["n_bad"] == h["n_bad"]
    assert dq <= golden["pose_bound"] and dt <= golden["pose_bound"]
