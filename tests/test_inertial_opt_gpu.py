"""Optimizer::InertialOptimization on the device (csrc/inertial_opt.hip) through the C ABI and its Python mirror against the
forward restatement of tests/inertial_opt_cases.py.

Bounds.  D is, per quantity (velocities relative to the scene's median speed, bg, ba, the entries of Rwg, scale, the per-edge chi2
relative to max(chi2, 1)), the largest difference between the forward restatement and any of its variants (three summation
orders, three solvers, a libm one ulp off, two orthonormalisations, two ways to the information matrix) over these very scenes:
tests/golden/inertial_opt_sensitivity.json, re-checked by tests/test_inertial_opt_cpu.py.  The device adds in one more order and has
another libm, so it may differ from the restatement by 16 D (DESIGN.md sections 10 to 19).  Status and the number of active edges
are equal in every scene; the iteration and rejected-trial counts are equal where the golden file says the variants agree, and
where a run has another length than the restatement's (possible only in the other scenes) the estimates are not compared: it is
another computation.  Device against the host program (the same header through g++ and glibc): the same bounds; byte-equality is
printed, not required.  Measured on an MI355X: DESIGN.md section 19."""
import os
import subprocess

import numpy as np
import pytest

import inertial_opt_cases as ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(msorb_mod, sc, **kw):
    r = msorb_mod.inertial_optimization(sc["problem"], sc["kfs"], sc["edges"], **kw)
    return r, ic.as_result(r["result"], r["v"], r["edge_chi2"])


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    d = tmp_path_factory.mktemp("inertial_opt_gpu")
    exe = str(d / "inertial_opt_main")
    b = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", os.path.join(ROOT, "tests", "inertial_opt_main.cc"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    scenes = [ic.scene(n) for n in ic.GPU_SCENES]
    ic.write_scenes(str(d / "in.bin"), scenes)
    p = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-2000:])
    return dict(zip(ic.GPU_SCENES, ic.read_results(str(d / "out.bin"), scenes)))


def _compare(name, r, other, what):
    g, b = ic.golden(), ic.bounds()
    d = ic.differences(r, other, ic.scene(name)["truth"]["speed"])
    print(f"{name}: device / {what}: counts {ic.counts(r)} / {ic.counts(other)}, in D: "
          + " ".join(f"{q} {d[q] / g['D'][q]:.4f}" for q in ic.QUANTITIES if g["D"][q] > 0)
          + f"; chi2 {r['chi2_initial']:.9e} -> {r['chi2_final']:.9e} / {other['chi2_initial']:.9e} -> {other['chi2_final']:.9e}")
    assert (r["status"], r["n_active_edges"]) == (other["status"], other["n_active_edges"])
    if g["scenes"][name]["counts_agree"]:
        assert ic.counts(r) == ic.counts(other)
    if ic.counts(r) == ic.counts(other):
        assert ic.within(d, b), (d, b)


@pytest.mark.parametrize("name", ic.GPU_SCENES)
def test_against_the_restatement(msorb_mod, host_results, name):
    sc = ic.scene(name)
    raw, r = _run(msorb_mod, sc)
    again, _ = _run(msorb_mod, sc)
    _compare(name, r, ic.reference(name), "restatement")
    _compare(name, r, host_results[name], "host program")
    same = all(np.array_equal(r[k], host_results[name][k]) for k in ("v", "bg", "ba", "Rwg", "chi2"))
    print(f"{name}: byte-equal to the host program: {same}")
    # a second run returns the same bits
    assert raw["v"].tobytes() == again["v"].tobytes() and raw["result"].tobytes() == again["result"].tobytes()
    assert raw["edge_chi2"].tobytes() == again["edge_chi2"].tobytes()
    # a KeyFrame without an edge has no active vertex: its velocity comes back as it went in
    lonely = np.setdiff1d(np.arange(len(sc["kfs"])), ic.chains(sc)[0])
    assert raw["v"][lonely].tobytes() == sc["kfs"]["v"][lonely].tobytes()
    if name in ("lonely_keyframe", "lonely_in_the_middle", "no_edges_first", "no_edges_third"):
        assert len(lonely) > 0


def _refused(msorb_mod, code, problem, kfs, edges):
    out = np.full((max(len(kfs), 1), 3), -7.0)
    with pytest.raises(msorb_mod.MsorbError) as e:
        msorb_mod.inertial_optimization(problem, kfs, edges, v_out=out)
    assert e.value.code == code and (out == -7.0).all()
    assert "inertial_optimization:" in str(e.value)              # msorb_last_error()'s text


def test_refusals_leave_the_device_usable(msorb_mod):
    sc = ic.scene("k9_mono")
    P, kfs, edges = sc["problem"], sc["kfs"], sc["edges"]
    INV, CAP = msorb_mod.E_INVALID, msorb_mod.E_CAPACITY
    for field, index, value in (("kf_prev", 2, len(kfs)), ("kf_cur", 0, -1), ("kf_cur", 3, int(edges["kf_prev"][3]))):   # indices
        bad = edges.copy()
        bad[field][index] = value
        _refused(msorb_mod, INV, P, kfs, bad)
    bad = edges.copy()
    bad["kf_prev"][5] = 0                                         # KeyFrame 0 with two outgoing edges: a fork
    _refused(msorb_mod, CAP, P, kfs, bad)
    bad = np.concatenate([edges, edges[:1]])
    bad["kf_prev"][-1], bad["kf_cur"][-1] = len(kfs) - 1, 0       # the chain closed into a cycle
    _refused(msorb_mod, CAP, P, kfs, bad)
    for field, value in (("dV", np.nan), ("info", np.inf), ("dT", np.nan)):
        bad = edges.copy()
        if field == "dT":
            bad[field][1] = value
        else:
            bad[field][1, 0] = value
        _refused(msorb_mod, INV, P, kfs, bad)
    badk = kfs.copy()
    badk["twb"][4, 1] = np.inf
    _refused(msorb_mod, INV, P, badk, edges)
    badk = kfs.copy()
    badk["has_velocity_vertex"][4] = 0                            # an edge whose vertex the reference would not find
    _refused(msorb_mod, INV, P, badk, edges)
    badp = P.copy()
    badp["scale"] = np.nan
    _refused(msorb_mod, INV, badp, kfs, edges)
    badp = P.copy()
    badp["algorithm"] = 2
    _refused(msorb_mod, INV, badp, kfs, edges)
    cap = msorb_mod.inertial_optimization_capacity()
    assert cap == 4096
    many = np.zeros(cap + 1, ic.KF_DTYPE)
    many["Rwb"], many["has_velocity_vertex"] = np.eye(3).reshape(9), 1
    _refused(msorb_mod, CAP, P, many, edges)
    import ctypes as C
    L = msorb_mod.lib()
    L.msorb_inertial_optimization.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
    out, res = np.full((len(kfs), 3), -7.0), np.zeros(1, ic.RESULT_DTYPE)
    p = lambda a: a.ctypes.data
    Pa, ka, ea = np.ascontiguousarray(P).reshape(1), np.ascontiguousarray(kfs), np.ascontiguousarray(edges)
    for args in ((0, None, len(ka), p(ka), len(ea), p(ea), p(out), None, p(res), None),               # null pointers
                 (0, p(Pa), len(ka), None, len(ea), p(ea), p(out), None, p(res), None),
                 (0, p(Pa), len(ka), p(ka), len(ea), None, p(out), None, p(res), None),
                 (0, p(Pa), len(ka), p(ka), len(ea), p(ea), None, None, p(res), None),
                 (0, p(Pa), len(ka), p(ka), len(ea), p(ea), p(out), None, None, None),
                 (0, p(Pa), -1, p(ka), len(ea), p(ea), p(out), None, p(res), None),                    # negative counts
                 (0, p(Pa), len(ka), p(ka), -1, p(ea), p(out), None, p(res), None)):
        assert L.msorb_inertial_optimization(*args) == INV and (out == -7.0).all()
    # one valid call afterwards passes
    _, r = _run(msorb_mod, sc)
    _compare("k9_mono", r, ic.reference("k9_mono"), "restatement after the refusals")


def test_exactly_at_the_capacity(msorb_mod):
    """4096 KeyFrames on a line at constant velocity, exact preintegrations: one Levenberg iteration runs and moves nothing far"""
    cap = msorb_mod.inertial_optimization_capacity()
    one = ic.make_scene(seed=1, K=2, mono=False, priors=(1e2, 1e5), noise=0.0)
    kfs = np.zeros(cap, ic.KF_DTYPE)
    kfs["Rwb"], kfs["has_velocity_vertex"] = one["kfs"]["Rwb"][0], 1
    edges = np.repeat(one["edges"], cap - 1)
    edges["kf_prev"], edges["kf_cur"] = np.arange(cap - 1), np.arange(1, cap)
    P = one["problem"].copy()
    P["iterations"] = 2
    r = msorb_mod.inertial_optimization(P, kfs, edges)
    assert int(r["result"]["status"]) == 0 and int(r["result"]["iterations"]) >= 1 and int(r["result"]["n_active_edges"]) == cap + 1
    assert np.isfinite(r["v"]).all() and np.isfinite(r["edge_chi2"]).all()
    assert float(r["result"]["chi2_final"]) <= float(r["result"]["chi2_initial"])
