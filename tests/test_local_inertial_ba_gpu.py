"""Optimizer::LocalInertialBA on the device (csrc/local_inertial_ba.hip) through the C ABI and its Python mirror, against the forward
restatement of tests/local_inertial_ba_cases.py and against the host program (the same header through g++ and glibc).

Bounds: those of tests/test_local_inertial_ba_cpu.py.  D is the largest difference between the forward restatement and any of its
variants over these very scenes (tests/golden/local_inertial_ba_sensitivity.json); the device has another libm, so it may differ
by 16 D (DESIGN.md sections 9 to 24).  Status, iterations, trials, rejected trials, the flags and their count are equal: the CPU
test shows that no compared chi2 comes within 100 times the chi2 spread of a threshold and no accept / reject decision within 100
times the cost spread.  Byte-equality with the host program is printed, not required.  The per-edge chi2 is NOT compared for the
device: the C ABI does not return it; tests/test_local_inertial_ba_cpu.py compares it for the host program.

Status 1: no scene of the list reaches the FAIL rule (the CPU test's docstring), so the arm is driven through its isnan() half: a
fixed KeyFrame whose finite but absurd camera rotation overflows the projection of the one point it sees."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import local_inertial_ba_cases as lc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = tuple(lc.GPU_SCENES)


def _args(sc):
    return (sc["kf"], sc["ie"], sc["pos"], sc["close"], sc["edge_kf"], sc["edge_pt"], sc["xy"], sc["ur"], sc["inv"])


def _run(msorb_mod, sc, **kw):
    return msorb_mod.local_inertial_ba(*_args(sc), large=bool(sc["large"]), iterations=int(sc["iterations"]), **kw)


def _as_result(r):
    return lc.from_records(r["result"], r["kf"], r["pos_d"], r["outlier"])


def nan_scene():
    """n2 plus a fixed KeyFrame whose Rcw is finite and overflows, seeing one point of its own: that edge's chi2 is NaN"""
    sc = lc.scene("n2")
    kf = np.concatenate([sc["kf"], sc["kf"][-1:]])
    kf[-1]["kind"] = 2
    kf[-1]["Rcw"] = 1.7e308
    P, K = len(sc["pos"]), len(kf)
    return dict(sc, kf=kf, pos=np.concatenate([sc["pos"], np.array([[2, 3, 5]], np.float32)]), close=np.concatenate([sc["close"], [0]]).astype(np.uint8),
                edge_kf=np.concatenate([sc["edge_kf"], [K - 1]]).astype(np.int32), edge_pt=np.concatenate([sc["edge_pt"], [P]]).astype(np.int32),
                xy=np.concatenate([sc["xy"], np.array([[100, 100]], np.float32)]), ur=np.concatenate([sc["ur"], [-1]]).astype(np.float32),
                inv=np.concatenate([sc["inv"], [1]]).astype(np.float32), iterations=2)


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    d = tmp_path_factory.mktemp("local_inertial_ba_gpu")
    exe = str(d / "local_inertial_ba_main")
    b = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", os.path.join(ROOT, "tests", "local_inertial_ba_main.cc"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    names = ALL + ("nan",)
    scenes = [lc.scene(n) for n in ALL] + [nan_scene()]
    lc.write_scenes(str(d / "in.bin"), scenes)
    p = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-2000:])
    return dict(zip(names, lc.read_results(str(d / "out.bin"), scenes)))


def test_capacity_and_records_are_what_the_scenes_assume(msorb_mod):
    assert msorb_mod.local_inertial_ba_capacity() == lc.CAPACITY >= 25
    assert (msorb_mod.IBA_PROBLEM_DTYPE, msorb_mod.IBA_KF_DTYPE, msorb_mod.IBA_EDGE_DTYPE, msorb_mod.IBA_KF_OUT_DTYPE, msorb_mod.IBA_RESULT_DTYPE) == (
        lc.PROBLEM_DTYPE, lc.KF_DTYPE, lc.IEDGE_DTYPE, lc.KF_OUT_DTYPE, lc.RESULT_DTYPE)


def _compare(name, sc, r, other, what):
    g, b = lc.golden(), lc.bounds()
    d = lc.differences(other, r, sc)
    d.pop("chi2")                                                              # (the device returns no per-edge chi2: nothing was compared)
    print(f"{name}: device / {what}: {lc.decisions(r)[:5]} / {lc.decisions(other)[:5]}, in D: " + " ".join(f"{q} {d[q] / g['D'][q]:.3f}" for q in d))
    assert lc.decisions(r) == lc.decisions(other), (name, what)
    assert lc.within(d, b), (name, what, d, b)


@pytest.mark.parametrize("name", ALL)
def test_device_against_the_restatement_and_the_host_program(msorb_mod, host_results, name):
    sc = lc.scene(name)
    out = _run(msorb_mod, sc)
    r = _as_result(out)
    _compare(name, sc, r, lc.reference(name), "restatement")
    rec, ko, h = host_results[name]
    _compare(name, sc, r, h, "host program")
    same = out["kf"].tobytes() == ko.tobytes() and np.array_equal(out["pos_d"], h["pts"]) and out["result"].tobytes() == rec.tobytes()
    print(f"{name}: device == host program bytes: {same}")
    # a second call returns the same bits
    again = _run(msorb_mod, sc)
    for k in ("kf", "pos", "pos_d", "outlier"):
        assert out[k].tobytes() == again[k].tobytes(), (name, k)
    assert out["result"].tobytes() == again["result"].tobytes()
    # the narrowed outputs, the bias in the reference's order (acc, then gyro), a fixed KeyFrame's repeat its input
    kf = out["kf"]
    for k in ("Rcw", "tcw", "v"):
        assert np.array_equal(kf[k + "_f"], kf[k].astype(np.float32)), (name, k)
    assert np.array_equal(kf["bias_f"], np.concatenate([kf["ba"], kf["bg"]], 1).astype(np.float32))
    assert np.array_equal(out["pos"], out["pos_d"].astype(np.float32))
    fixed = sc["kf"]["kind"] != 0
    for k in ("Rwb", "twb", "Rcw", "tcw", "v", "bg", "ba"):
        assert np.array_equal(kf[k][fixed], sc["kf"][k][fixed]), (name, k)
    assert int(out["result"]["n_outliers"]) == int(out["outlier"].sum())
    assert out["result"]["err"] == np.float32(out["result"]["chi2_initial"]) and out["result"]["err_end"] == np.float32(out["result"]["chi2_final"])


def _outputs_repeat_inputs(sc, out):
    for k in ("Rwb", "twb", "Rcw", "tcw", "v", "bg", "ba"):
        assert np.array_equal(out["kf"][k], sc["kf"][k]), k
    assert np.array_equal(out["kf"]["Rcw_f"], sc["kf"]["Rcw"].astype(np.float32))
    assert np.array_equal(out["pos"], sc["pos"]) and np.array_equal(out["pos_d"], sc["pos"].astype(np.float64)) and not out["outlier"].any()


def test_status_1_and_status_2_leave_every_output_equal_to_its_input(msorb_mod, host_results):
    sc = nan_scene()
    with np.errstate(all="ignore"):
        ref = lc.optimize(sc)
    out = _run(msorb_mod, sc)
    rec = host_results["nan"][0]
    print("nan scene: device", out["result"], "host program", rec, "restatement", lc.decisions(ref)[:4])
    assert int(out["result"]["status"]) == 1 == int(rec["status"]) == ref["status"] and np.isnan(out["result"]["err"])
    assert [int(out["result"][k]) for k in ("iterations", "trials", "rejected_trials")] == [ref[k] for k in ("iterations", "trials", "rejected_trials")]
    assert int(out["result"]["n_outliers"]) == 0
    _outputs_repeat_inputs(sc, out)
    large = _run(msorb_mod, dict(sc, large=1))                                  # bLarge switches the FAIL rule off
    assert int(large["result"]["status"]) == 0 and np.isnan(large["result"]["err"])
    # status 2: fixed KeyFrames only and no edge
    base = lc.scene("n2")
    kf = base["kf"].copy()
    kf["kind"] = np.where(kf["kind"] == 0, 1, kf["kind"])
    e = np.zeros(0, np.int32)
    f = np.zeros(0, np.float32)
    sc2 = dict(base, kf=kf, edge_kf=e, edge_pt=e, xy=np.zeros((0, 2), np.float32), ur=f, inv=f)
    out = _run(msorb_mod, sc2)
    assert int(out["result"]["status"]) == 2 and int(out["result"]["iterations"]) == 0
    _outputs_repeat_inputs(sc2, out)
    assert lc.optimize(sc2)["status"] == 2


def test_three_host_threads_on_different_scenes(msorb_mod):
    names = ("n3", "mixed", "n10")
    single = {n: _run(msorb_mod, lc.scene(n)) for n in names}
    got, errors = {}, []

    def work(n):
        try:
            for _ in range(3):
                got[n] = _run(msorb_mod, lc.scene(n))
        except Exception as e:  # noqa: BLE001
            errors.append((n, e))
    threads = [threading.Thread(target=work, args=(n,)) for n in names]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for n in names:
        for k in ("kf", "pos_d", "outlier"):
            assert got[n][k].tobytes() == single[n][k].tobytes(), (n, k)
        assert got[n]["result"].tobytes() == single[n]["result"].tobytes()


def _sentinels(sc):
    K, P, E = len(sc["kf"]), len(sc["pos"]), len(sc["edge_kf"])
    kf = np.zeros(max(K, 1), lc.KF_OUT_DTYPE)
    kf.view(np.uint8)[:] = 0xA5
    return (kf, np.full((max(P, 1), 3), 7.5, np.float32), np.full((max(P, 1), 3), 7.5), np.full(max(E, 1), 9, np.uint8))


def _refused(msorb_mod, sc, code):
    out = _sentinels(sc)
    before = [a.copy() for a in out]
    with pytest.raises(msorb_mod.MsorbError) as ei:
        _run(msorb_mod, sc, out=out)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    for a, b in zip(out, before):
        assert a.tobytes() == b.tobytes()


def test_one_more_free_keyframe_than_the_capacity(msorb_mod):
    sc = lc.build(900, lc.CAPACITY + 1, 30, n_fixed=1, large=True)
    assert (sc["kf"]["kind"] == 0).sum() == lc.CAPACITY + 1
    _refused(msorb_mod, sc, -4)
    # edges that do not form chains are "not handled" too
    base = lc.scene("n3")
    ie = np.concatenate([base["ie"], base["ie"][-1:]])
    _refused(msorb_mod, dict(base, ie=ie), -4)


def test_every_argument_error_is_refused_with_nothing_written(msorb_mod):
    base = lc.scene("n3")
    K, P = len(base["kf"]), len(base["pos"])

    def edit(key, fn):
        a = base[key].copy()
        fn(a)
        return dict(base, **{key: a})

    def set_at(i, v):
        return lambda a: a.__setitem__(i, v)
    cases = {
        "edge_kf out of range": edit("edge_kf", set_at(5, K)),
        "edge_kf negative": edit("edge_kf", set_at(5, -1)),
        "edge_point out of range": edit("edge_pt", set_at(-1, P)),
        "not point-major": edit("edge_pt", lambda a: a.__setitem__(slice(None), a[::-1].copy())),
        "non-finite point": edit("pos", set_at((3, 1), np.nan)),
        "non-finite observation": edit("xy", set_at((0, 0), np.inf)),
        "non-finite weight": edit("inv", set_at(0, np.nan)),
        "unknown kind": edit("kf", lambda a: a["kind"].__setitem__(1, 3)),
        "non-finite KeyFrame": edit("kf", lambda a: a["twb"].__setitem__((1, 0), np.nan)),
        "inertial edge out of range": edit("ie", lambda a: a["pre"]["kf_cur"].__setitem__(0, K)),
        "inertial edge to itself": edit("ie", lambda a: a["pre"]["kf_cur"].__setitem__(0, int(a["pre"]["kf_prev"][0]))),
        "inertial edge on a kind 2 KeyFrame": edit("ie", lambda a: a["pre"]["kf_cur"].__setitem__(2, K - 1)),
        "non-finite information": edit("ie", lambda a: a["pre"]["info"].__setitem__((1, 4), np.nan)),
        "negative iterations": dict(base, iterations=-1),
    }
    assert base["kf"]["kind"][K - 1] == 2
    for what, sc in cases.items():
        print(what)
        _refused(msorb_mod, sc, -1)
    # a null required pointer and a negative count need the C entry itself
    L = msorb_mod.lib()
    out = _sentinels(base)
    before = [a.copy() for a in out]
    res = np.zeros(1, lc.RESULT_DTYPE)
    pr = np.zeros(1, lc.PROBLEM_DTYPE)
    ptr = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)  # noqa: E731
    keep = [np.ascontiguousarray(a) for a in _args(base)]
    kf, ie, pos, close, ek, ep, xy, ur, inv = keep
    full = [0, ptr(pr), K, ptr(kf), len(ie), ptr(ie), P, ptr(pos), ptr(close), len(ek), ptr(ek), ptr(ep), ptr(xy), ptr(ur), ptr(inv),
            ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(res), None]
    L.msorb_local_inertial_ba.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_int] + [C.c_void_p] * 11
    for i in (1, 3, 5, 7, 8, 10, 11, 12, 13, 14, 15, 16, 18, 19):              # every required pointer (pos_d and elapsed_ms are optional)
        a = list(full)
        a[i] = None
        assert L.msorb_local_inertial_ba(*a) == -1, i
    for i in (2, 4, 6, 9):
        a = list(full)
        a[i] = -1
        assert L.msorb_local_inertial_ba(*a) == -1, i
    for a, b in zip(out, before):
        assert a.tobytes() == b.tobytes()
    assert not res.view(np.uint8).any()
