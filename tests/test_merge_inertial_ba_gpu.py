"""Optimizer::MergeInertialBA on the device (csrc/inertial_ba_engine.hip) through the C ABI and its Python mirror, against the forward
restatement of tests/merge_inertial_ba_cases.py and against the host program (the same header through g++ and glibc, a serial
executor, the column-by-column solve).

Bounds: those of tests/test_merge_inertial_ba_cpu.py: 16 D, D from tests/golden/merge_inertial_ba_sensitivity.json; status,
iterations, trials, rejected trials, every outlier flag and point_included are equal (the CPU test shows that no accept / reject
decision and no classification comes within 100 times the spread).  Byte-equality with the host program is printed, not required.
The two scenes whose stop flag is raised by a hand-made hook in mid-call (stop_trial, stop_iteration) run in the host program only:
the C entry polls a flag it is given, and a flag that is set before the call is tested here."""
import os
import subprocess

import numpy as np
import pytest

import full_inertial_ba_cases as fc
import local_inertial_ba_cases as lc
import merge_inertial_ba_cases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = mc.DEVICE


def _args(sc):
    return (sc["kf"], sc["ie"], sc["pos"], sc["edge_kf"], sc["edge_pt"], sc["xy"], sc["ur"], sc["inv"])


def _run(msorb_mod, sc, **kw):
    if sc.get("stop_trials", -1) == 0:
        kw.setdefault("stop_flag", np.ones(1, np.int32))
    return msorb_mod.merge_inertial_ba(*_args(sc), iterations=int(sc["iterations"]), **kw)


def _as_result(r):
    return mc.from_records(r["result"], r["kf"], r["pos_d"], r["outlier"], r["included"])


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    d = tmp_path_factory.mktemp("merge_inertial_ba_gpu")
    exe = str(d / "merge_inertial_ba_main")
    b = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", os.path.join(ROOT, "tests", "merge_inertial_ba_main.cc"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    scenes = [mc.scene(n) for n in ALL]
    mc.write_scenes(str(d / "in.bin"), scenes)
    p = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-2000:])
    return dict(zip(ALL, mc.read_results(str(d / "out.bin"), scenes)))


def test_capacity_and_records_are_what_the_scenes_assume(msorb_mod):
    assert msorb_mod.merge_inertial_ba_capacity() == mc.CAPACITY == 7168
    assert msorb_mod.IBA_KF_DTYPE == lc.KF_DTYPE and msorb_mod.IBA_RESULT_DTYPE == lc.RESULT_DTYPE
    assert all(hasattr(msorb_mod.lib(), s) for s in ("msorb_merge_inertial_ba", "msorb_merge_inertial_ba_capacity", "msorb_merge_inertial_ba_stage_ms"))


def _compare(name, sc, r, other, what):
    D = mc.golden()["D"]
    d = mc.differences(other, r, sc)
    print(f"{name}: device / {what}: {mc.decisions(r)[:4]} / {mc.decisions(other)[:4]}, flagged {int(r['flags'].sum())}, in D: "
          + " ".join(f"{q} {d[q] / D[q]:.3f}" for q in d if D[q] > 0))
    assert mc.decisions(r) == mc.decisions(other), (name, what)
    assert mc.within(d, mc.bounds()), (name, what, d, mc.bounds())


@pytest.mark.parametrize("name", ALL)
def test_device_against_the_restatement_and_the_host_program(msorb_mod, host_results, name):
    sc = mc.scene(name)
    out = _run(msorb_mod, sc)
    r = _as_result(out)
    _compare(name, sc, r, mc.reference(name), "restatement")
    rec, ko, h = host_results[name]
    _compare(name, sc, r, h, "host program")
    same = out["kf"].tobytes() == ko.tobytes() and np.array_equal(out["pos_d"], h["pts"]) and out["result"].tobytes() == rec.tobytes()
    print(f"{name}: device == host program bytes: {same}")
    # a second call returns the same bits
    again = _run(msorb_mod, sc)
    for k in ("kf", "pos", "pos_d", "outlier", "included"):
        assert out[k].tobytes() == again[k].tobytes(), (name, k)
    assert out["result"].tobytes() == again["result"].tobytes()
    # the narrowed outputs, the bias in the reference's order (acc, then gyro)
    kf, kind = out["kf"], sc["kf"]["kind"]
    for k in ("Rcw", "tcw", "v"):
        assert np.array_equal(kf[k + "_f"], kf[k].astype(np.float32)), (name, k)
    assert np.array_equal(kf["bias_f"], np.concatenate([kf["ba"], kf["bg"]], 1).astype(np.float32))
    assert np.array_equal(out["pos"], out["pos_d"].astype(np.float32))
    # a fixed KeyFrame repeats its input; a pose-only KeyFrame repeats v, bg, ba and, where an edge reaches it, its pose moved
    fixed = (kind == 1) | (kind == 2)
    for k in ("Rwb", "twb", "Rcw", "tcw", "v", "bg", "ba"):
        assert np.array_equal(kf[k][fixed], sc["kf"][k][fixed]), (name, k)
    pose_only = kind == 3
    for k in ("v", "bg", "ba"):
        assert np.array_equal(kf[k][pose_only], sc["kf"][k][pose_only]), (name, k)
    status = int(out["result"]["status"])
    if status == 0:
        reached = np.zeros(len(kind), bool)
        reached[sc["edge_kf"]] = True
        moved = np.array([not np.array_equal(kf["tcw"][k], sc["kf"]["tcw"][k]) for k in range(len(kind))])
        assert moved[pose_only & reached].all() and not moved[pose_only & ~reached].any()
        assert moved[kind == 0].all()
    else:
        assert status == 3 and not out["outlier"].any() and not out["included"].any() and np.array_equal(kf["tcw"], sc["kf"]["tcw"])
    left_out = ~out["included"]
    assert np.array_equal(out["pos"][left_out], sc["pos"][left_out]) and not out["outlier"][left_out[sc["edge_pt"]]].any()
    assert int(out["result"]["n_outliers"]) == int(out["outlier"].sum()) and out["result"]["err"] == 0 and int(out["result"]["reserved"]) == 0


def test_a_point_behind_its_camera_with_a_small_chi2_is_not_flagged(msorb_mod):
    sc = mc.scene("depth_negative")
    out = _run(msorb_mod, sc)
    e = int(np.flatnonzero(sc["edge_pt"] == 0)[0])
    k = int(sc["edge_kf"][e])
    z = out["kf"]["Rcw"][k].reshape(3, 3)[2] @ out["pos_d"][0] + out["kf"]["tcw"][k][2]
    assert z < -1.0 and out["included"][0] and not out["outlier"][e] and out["outlier"].any()


def _outputs_repeat_inputs(sc, out):
    for k in ("Rwb", "twb", "Rcw", "tcw", "v", "bg", "ba"):
        assert np.array_equal(out["kf"][k], sc["kf"][k]), k
    assert np.array_equal(out["kf"]["Rcw_f"], sc["kf"]["Rcw"].astype(np.float32))
    assert np.array_equal(out["pos"], sc["pos"]) and np.array_equal(out["pos_d"], sc["pos"].astype(np.float64))
    assert not out["included"].any() and not out["outlier"].any()


def test_status_2_and_status_3_leave_every_output_equal_to_its_input(msorb_mod):
    sc = mc.scene("small")
    out = _run(msorb_mod, sc, stop_flag=np.ones(1, np.int32))                  # the flag is set before optimize()
    assert int(out["result"]["status"]) == 3 and int(out["result"]["iterations"]) == 0 and int(out["result"]["trials"]) == 0
    _outputs_repeat_inputs(sc, out)
    clear = _run(msorb_mod, sc, stop_flag=np.zeros(1, np.int32))               # a flag that stays clear changes nothing
    assert clear["kf"].tobytes() == _run(msorb_mod, sc)["kf"].tobytes() and int(clear["result"]["status"]) == 0
    kf = sc["kf"].copy()                                                       # status 2: no free KeyFrame
    kf["kind"] = 1
    sc2 = dict(sc, kf=kf)
    out = _run(msorb_mod, sc2)
    assert int(out["result"]["status"]) == 2 and mc.optimize(sc2)["status"] == 2
    _outputs_repeat_inputs(sc2, out)
    # status 2: free KeyFrames that no edge reaches are no vertices
    sc3 = dict(sc, ie=sc["ie"][:0], edge_kf=sc["edge_kf"][:0], edge_pt=sc["edge_pt"][:0], xy=sc["xy"][:0], ur=sc["ur"][:0], inv=sc["inv"][:0])
    out = _run(msorb_mod, sc3)
    assert int(out["result"]["status"]) == 2 and mc.optimize(sc3)["status"] == 2
    _outputs_repeat_inputs(sc3, out)


def _sentinels(sc):
    K, P, E = len(sc["kf"]), len(sc["pos"]), len(sc["edge_kf"])
    kf = np.zeros(max(K, 1), lc.KF_OUT_DTYPE)
    kf.view(np.uint8)[:] = 0xA5
    return (kf, np.full((max(P, 1), 3), 7.5, np.float32), np.full((max(P, 1), 3), 7.5), np.full(max(E, 1), 9, np.uint8), np.full(max(P, 1), 9, np.uint8))


def _refused(msorb_mod, sc, code):
    out = _sentinels(sc)
    before = [a.copy() for a in out]
    with pytest.raises(msorb_mod.MsorbError) as ei:
        _run(msorb_mod, sc, out=out)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    for a, b in zip(out, before):
        assert a.tobytes() == b.tobytes()


def test_graphs_and_inputs_that_are_refused_with_nothing_written(msorb_mod):
    s = mc.scene("small")
    K = len(s["kf"])
    ie = s["ie"].copy()
    ie[0]["pre"]["kf_cur"] = K - 1                                             # an inertial edge on a kind 3 KeyFrame
    assert s["kf"]["kind"][K - 1] == 3 and mc.validate(dict(s, ie=ie)) == "invalid"
    _refused(msorb_mod, dict(s, ie=ie), -1)
    fork = np.concatenate([s["ie"], s["ie"][:1]])                              # two edges leave KeyFrame 0
    fork[-1]["pre"]["kf_cur"] = 3
    assert mc.validate(dict(s, ie=fork)) == "capacity"
    _refused(msorb_mod, dict(s, ie=fork), -4)
    cyc = s["ie"][2:4].copy()                                                  # 3 -> 4 -> 5 closed by 5 -> 3
    extra = cyc[:1].copy()
    extra[0]["pre"]["kf_prev"], extra[0]["pre"]["kf_cur"] = 5, 3
    cyc = np.concatenate([cyc, extra])
    assert mc.validate(dict(s, ie=cyc)) == "capacity"
    _refused(msorb_mod, dict(s, ie=cyc), -4)
    for key, at in (("pos", (3, 1)), ("xy", (0, 0)), ("inv", 0)):              # a non-finite input
        a = s[key].copy()
        a[at] = np.nan
        _refused(msorb_mod, dict(s, **{key: a}), -1)
    kf = s["kf"].copy()
    kf["twb"][1, 0] = np.inf
    _refused(msorb_mod, dict(s, kf=kf), -1)
    kf = s["kf"].copy()
    kf["kind"][1] = 4                                                          # an unknown kind
    _refused(msorb_mod, dict(s, kf=kf), -1)
    _refused(msorb_mod, dict(s, iterations=-1), -1)


def test_the_smallest_graph_above_the_capacity(msorb_mod):
    """6 a + 15 b is a multiple of 3 and 7168 is not: the largest graph that fits has 7167 unknowns (1192 pose-only KeyFrames and one of
    kind 0), the smallest that does not has 7170 (1190 and two).  The check reads the records and the edges' indices and nothing else."""
    base = mc.scene("small")

    def graph_of(n3, n0):
        kf = np.zeros(1 + n0 + n3, lc.KF_DTYPE)                                # [kind 1 | n0 of kind 0 along one chain | n3 of kind 3]
        kf["kind"][0], kf["kind"][1 + n0:] = 1, 3
        ie = base["ie"][:n0].copy()
        ie["pre"]["kf_prev"], ie["pre"]["kf_cur"] = np.arange(n0), np.arange(1, n0 + 1)
        ek = np.arange(1 + n0, 1 + n0 + n3, dtype=np.int32)                    # one point seen by every pose-only KeyFrame
        return dict(base, kf=kf, ie=ie, pos=np.zeros((1, 3), np.float32), edge_kf=ek, edge_pt=np.zeros(n3, np.int32),
                    xy=np.zeros((n3, 2), np.float32), ur=np.full(n3, -1, np.float32), inv=np.ones(n3, np.float32))
    fits = graph_of(1192, 1)
    assert mc.graph(fits)["n"] == mc.CAPACITY - 1 and mc.validate(fits) is None
    sc = graph_of(1190, 2)
    assert mc.graph(sc)["n"] == mc.CAPACITY + 2 and mc.validate(sc) == "capacity"
    _refused(msorb_mod, sc, -4)


def test_the_other_two_entries_still_refuse_kind_3(msorb_mod):
    s = mc.scene("small")
    assert (s["kf"]["kind"] == 3).any()
    with pytest.raises(msorb_mod.MsorbError) as ei:
        msorb_mod.local_inertial_ba(s["kf"], s["ie"], s["pos"], np.zeros(len(s["pos"]), np.uint8), s["edge_kf"], s["edge_pt"], s["xy"], s["ur"], s["inv"],
                                    iterations=1)
    assert ei.value.code == -1
    with pytest.raises(msorb_mod.MsorbError) as ei:
        msorb_mod.full_inertial_ba(s["kf"], s["ie"], s["pos"], s["edge_kf"], s["edge_pt"], s["xy"], s["ur"], s["inv"], iterations=1)
    assert ei.value.code == -1


def test_both_routines_interleaved_on_one_thread_return_the_bytes_of_a_call_alone(msorb_mod):
    """FullInertialBA and MergeInertialBA share one device block, one pinned block, one stream and one pool of events per thread.  The
    sequence grows the block, makes a smaller call of the other layout read what a larger one left in it, and comes back."""
    def full(name):
        sc = fc.scene(name)
        return msorb_mod.full_inertial_ba(*_args(sc), init=bool(sc["init"]), iterations=int(sc["iterations"]), prior_g=sc["prior_g"],
                                          prior_a=sc["prior_a"], bg0=sc["bg0"], ba0=sc["ba0"])
    calls = {"f1": full, "i1": full, "f16": full, "small": lambda n: _run(msorb_mod, mc.scene(n)),
             "pose_only_many": lambda n: _run(msorb_mod, mc.scene(n))}

    def kept(name):
        out = calls[name](name)
        assert int(out["result"]["status"]) == 0, name
        return {k: out[k].tobytes() for k in ("kf", "pos", "pos_d", "included", "result", "outlier") if k in out}
    alone = {name: kept(name) for name in calls}
    assert all(("outlier" in alone[n]) == (n in ("small", "pose_only_many")) for n in alone)
    for i, name in enumerate(("f16", "small", "i1", "pose_only_many", "f1", "small", "f16")):
        got = kept(name)
        for k in alone[name]:
            assert got[k] == alone[name][k], (i, name, k)
