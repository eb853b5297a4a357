"""Both overloads of msorb_host::OptimizeSim3 (ms-slam_amd/host/Optimizer_device.h) compiled against the stand-ins of tests/slam_stub
(tests/dropin_sim3opt_main.cc): which matches are reset, the return value, g2oS12 written only when the second optimisation was
made, the zeroed Hessian, the skip rules of the gathering loops (by counting the gathered pairs) and the -1 answers, against the
restatement of tests/sim3_opt_cases.py fed with the arrays the C++ side gathered (R * Xw + t there is the caller's arithmetic)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import sim3_opt_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAS1, MATCH, BAD1, BAD2, IN_KF2 = 1, 2, 4, 8, 16
GOOD = HAS1 | MATCH | IN_KF2
INV_SIGMA2 = (1.0 / (1.2 ** np.arange(8)) ** 2).astype(np.float32)
LOG_SCALE = np.float32(np.log(1.2))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("dropin_sim3opt") / "dropin_sim3opt"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", f"-I{ROOT}/tests/slam_stub", f"-I{ROOT}/tests/cv_stub",
                           f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include", f"{ROOT}/tests/dropin_sim3opt_main.cc", f"-L{ROOT}/ms-slam_amd",
                           "-lmsorb", f"-Wl,-rpath,{ROOT}/ms-slam_amd", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def golden():
    with open(sc.GOLDEN) as f:
        return json.load(f)


def _rot(rng, angle):
    q = sc._quat_from_axis_angle(rng.normal(size=3), angle)
    return np.stack([sc.rotate(q, np.eye(3)[k]) for k in range(3)], -1)      # columns = the rotated unit vectors


def _case(seed, n, fix_scale, n_good=None, outliers=0.25):
    """a scene of sim3_opt_cases behind two KeyFrame poses, with every reason to skip an entry mixed in"""
    rng = np.random.RandomState(seed)
    s = sc.make_scene(seed, n, outliers=outliers, fix_scale=fix_scale, cam2=sc.CAM_B)
    flags = np.full(n, GOOD, np.int32)
    if n_good is None:
        spoil = [HAS1, MATCH | IN_KF2, GOOD | BAD1, GOOD | BAD2, GOOD & ~IN_KF2]
        at = rng.permutation(n - 1)[:4 * len(spoil)]
        flags[at] = np.tile(spoil, 4)
    else:
        flags[n_good:] = HAS1
    poses = [(_rot(rng, 0.4 * (k + 1)).astype(np.float32), rng.uniform(-1, 1, 3).astype(np.float32)) for k in range(2)]
    Xc = [s["P1c"].astype(np.float64), s["P2c"].astype(np.float64)]
    behind = n - 1                                                             # a good entry whose P3D2c lies behind KeyFrame 2 (:2100)
    Xc[1][behind, 2] = -2.0
    Xw = [((X - t.astype(np.float64)) @ R.astype(np.float64)).astype(np.float32) for X, (R, t) in zip(Xc, poses)]   # R^T (Xc - t)
    return dict(s=s, n=n, fix_scale=fix_scale, flags=flags, poses=poses, Xw=Xw, behind=behind,
                oct=[rng.randint(0, 8, n).astype(np.int32) for _ in range(2)], track_level=rng.randint(0, 8, n).astype(np.int32),
                max_dist=[(np.linalg.norm(X, axis=1) * rng.uniform(1.0, 3.0, n)).astype(np.float32) for X in Xc])


def _run(exe, tmp_path, c, overload, all_points=0, spoil=0):
    s, n = c["s"], c["n"]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<5if", overload, int(c["fix_scale"]), all_points, spoil, n, s["th2"]))
        for k in range(2):
            R, t = c["poses"][k]
            f.write(np.ascontiguousarray(R).tobytes() + t.tobytes() + np.asarray(s["cam1" if k == 0 else "cam2"], np.float32).tobytes() +
                    INV_SIGMA2.tobytes() + LOG_SCALE.tobytes())
        f.write(np.concatenate([s["q"], s["t"], [s["s"]]]).astype(np.float64).tobytes())
        for i in range(n):
            f.write(struct.pack("<4i", int(c["flags"][i]), int(c["oct"][0][i]), int(c["oct"][1][i]), int(c["track_level"][i])))
            f.write(c["Xw"][0][i].tobytes() + c["Xw"][1][i].tobytes() + s["obs1"][i].astype(np.float32).tobytes() +
                    s["obs2"][i].astype(np.float32).tobytes() + struct.pack("<2f", c["max_dist"][0][i], c["max_dist"][1][i]))
    subprocess.check_call([exe, fin, fout], timeout=120)
    raw = open(fout, "rb").read()
    ret, handled, m, ncorr = struct.unpack_from("<4i", raw)
    off = 16
    G = {}
    for key, w in (("P1c", 3), ("P2c", 3), ("obs1", 2), ("obs2", 2), ("w1", 1), ("w2", 1)):
        G[key] = np.frombuffer(raw, np.float32, w * m, off).reshape(m, w) if w > 1 else np.frombuffer(raw, np.float32, m, off)
        off += 4 * w * m
    index = np.frombuffer(raw, np.int32, m, off)
    off += 4 * m
    m1 = np.frombuffer(raw, np.uint8, n, off).astype(bool)
    m2 = np.frombuffer(raw, np.uint8, n, off + n).astype(bool)
    off += 2 * n
    S = np.frombuffer(raw, np.float64, 8, off)
    H = np.frombuffer(raw, np.float64, 49, off + 64)
    return dict(ret=ret, handled=handled, G=G, index=index, ncorr=ncorr, matches1=m1, matches2=m2, S=S, H=H)


def _check(msorb_mod, golden, c, o, overload, all_points, min_pairs):
    s, flags, n = c["s"], c["flags"], c["n"]
    usable = ((flags & (HAS1 | MATCH)) == (HAS1 | MATCH)) & ((flags & (BAD1 | BAD2)) == 0)
    expect = usable.copy()
    if overload == 1:
        if not all_points:
            expect &= (flags & IN_KF2) != 0                                    # :2093
        expect[c["behind"]] = False                                            # :2100
    assert o["handled"] == 1 and o["index"].tolist() == np.flatnonzero(expect).tolist() and o["ncorr"] == len(o["index"])
    G, idx = o["G"], o["index"]
    # what the gathering loops hand over
    if overload == 1:
        assert np.array_equal(G["obs1"], s["obs1"][idx].astype(np.float32))
        assert np.array_equal(G["w1"], INV_SIGMA2[c["oct"][0][idx]])
        in2 = (flags[idx] & IN_KF2) != 0
        assert np.array_equal(G["obs2"][in2], s["obs2"][idx].astype(np.float32)[in2]) and np.array_equal(G["w2"][in2], INV_SIGMA2[c["oct"][1][idx]][in2])
        if all_points:
            assert (~in2).sum() >= 3
            invz = np.float32(1) / G["P2c"][~in2, 2]
            assert np.array_equal(G["obs2"][~in2], np.stack([G["P2c"][~in2, 0] * invz, G["P2c"][~in2, 1] * invz], -1))   # :2141-2145
            assert np.array_equal(G["w2"][~in2], INV_SIGMA2[c["track_level"][idx]][~in2])                              # mnTrackScaleLevel
    else:
        c1, c2 = np.asarray(s["cam1"], np.float32), np.asarray(s["cam2"], np.float32)
        for key, cam, P in (("obs1", c1, G["P1c"]), ("obs2", c2, G["P2c"])):     # pCamera->project in float
            assert np.array_equal(G[key], np.stack([cam[0] * P[:, 0] / P[:, 2] + cam[2], cam[1] * P[:, 1] / P[:, 2] + cam[3]], -1))
        assert len(set(G["w1"].tolist())) > 2 and set(G["w1"].tolist()) <= set(INV_SIGMA2.tolist())                  # PredictScale
    # the routine, on the gathered arrays
    args = (s["cam1"], s["cam2"], s["q"], s["t"], s["s"], G["P1c"], G["P2c"], G["obs1"], G["obs2"], G["w1"], G["w2"], s["th2"], c["fix_scale"], min_pairs)
    refs = [sc.optimize_sim3(*args, sum_order=v[0], nudge=v[1]) for v in sc.VARIANTS]
    ref = refs[0]
    margin = min(float(np.min(np.abs(x[np.isfinite(x)] - ref["th2"]) / ref["th2"])) for r in refs for x in r["chi2_read"] if x.size)
    print(f"overload {overload} all_points {all_points}: gathered {len(idx)} status {ref['status']} n_bad {ref['n_bad']} n_in {ref['n_in']} "
          f"margin {margin:.3e} ret {o['ret']}")
    assert margin > 100 * golden["C"]                                            # a scene closer to th2 is replaced, not tolerated
    p = msorb_mod.sim3_opt_problem(s["q"], s["t"], s["s"], s["cam1"], s["cam2"], s["th2"], c["fix_scale"], min_pairs, len(idx))
    dev, dev_bad, _ = msorb_mod.sim3_optimization_batch(p, G["P1c"], G["P2c"], G["obs1"], G["obs2"], G["w1"], G["w2"])
    assert np.array_equal(dev_bad, ref["bad"]) and int(dev[0]["status"]) == ref["status"]
    before1 = (flags & (MATCH if overload == 1 else HAS1)) != 0
    reset = np.zeros(n, bool)
    reset[idx[ref["bad"] != 0]] = True
    assert np.array_equal(o["matches1"], before1 & ~reset)                       # bad pairs reset, every other entry as it was
    if overload == 2:
        assert np.array_equal(o["matches2"], ((flags & MATCH) != 0) & ~reset)
    S_in = np.concatenate([s["q"], s["t"], [s["s"]]])
    if ref["status"] == 0:
        assert o["ret"] == ref["n_in"] and not o["H"].any()
        assert o["S"].tobytes() == np.concatenate([dev[0]["q"], dev[0]["t"], [dev[0]["s"]]]).tobytes()   # the entry's own bits
        got = dict(q=o["S"][:4], t=o["S"][4:7], s=float(o["S"][7]))
        assert sc.estimate_difference(got, ref, s["median_depth"]) <= golden["estimate_bound"]
    else:
        assert o["ret"] == 0 and (o["H"] == 7.0).all() and o["S"].tobytes() == S_in.tobytes()      # returned before either is written
    return ref


@pytest.mark.parametrize("all_points,fix_scale", [(0, False), (1, True)])
def test_first_overload(msorb_mod, golden, exe, tmp_path, all_points, fix_scale):
    c = _case(31 + all_points, 160, fix_scale)
    ref = _check(msorb_mod, golden, c, _run(exe, tmp_path, c, 1, all_points), 1, all_points, 10)
    assert ref["status"] == 0 and ref["n_bad"] > 0 and ref["n_in"] > 50


def test_second_overload(msorb_mod, golden, exe, tmp_path):
    c = _case(41, 120, False)
    ref = _check(msorb_mod, golden, c, _run(exe, tmp_path, c, 2), 2, 0, 5)
    assert ref["status"] == 0 and ref["n_bad"] > 0 and ref["n_in"] > 50


@pytest.mark.parametrize("overload,n_good", [(1, 9), (2, 4)])
def test_below_the_minimum_nothing_is_written(msorb_mod, golden, exe, tmp_path, overload, n_good):
    c = _case(50 + overload, 30, False, n_good=n_good, outliers=0.0)
    c["flags"][c["behind"]] = HAS1
    ref = _check(msorb_mod, golden, c, _run(exe, tmp_path, c, overload), overload, 0, 10 if overload == 1 else 5)
    assert ref["status"] == 1 and ref["n_pairs"] == n_good


@pytest.mark.parametrize("overload", [1, 2])
def test_minus_one_for_what_is_not_handled(exe, tmp_path, overload):
    c = _case(60, 40, False)
    S_in = np.concatenate([c["s"]["q"], c["s"]["t"], [c["s"]["s"]]])
    before1 = (c["flags"] & (MATCH if overload == 1 else HAS1)) != 0
    runs = [_run(exe, tmp_path, c, overload, spoil=1), _run(exe, tmp_path, c, overload, spoil=2)]
    if overload == 1:
        c["oct"][0][int(np.flatnonzero(c["flags"] == GOOD)[3])] = 11            # :2110 would leave a half-added edge
        runs.append(_run(exe, tmp_path, c, 1))
    for o in runs:
        assert o["ret"] == -1 and o["handled"] == 0
        assert np.array_equal(o["matches1"], before1) and o["S"].tobytes() == S_in.tobytes() and (o["H"] == 7.0).all()
