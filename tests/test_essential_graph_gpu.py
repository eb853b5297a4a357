"""Optimizer::OptimizeEssentialGraph on the device (csrc/essential_graph.hip) through the C ABI against the float64 restatement of
tests/essential_graph_cases.py ('forward' = g2o's order, the unpivoted L D L^T).

Bounds.  D is the largest difference between any two of the restatement's variants (three summation orders, a libm nudged by one
ulp, the system through LAPACK) on an estimate over these very scenes, committed in tests/golden/essential_graph_sensitivity.json
and re-checked by tests/test_essential_graph_cpu.py.  The device adds in one more order and has another libm, so its estimates
may differ from the restatement's by 16 D (DESIGN.md sections 10, 14, 16, 17), and, since D is set by the 150-vertex scene alone, by no
more than 16 times the scene's own recorded spread (essential_graph_cases.scene_bound).  Counts, status and solver flags are equal: no
scene is left out, every scene here is one on which all variants agree.

Device against the host program (the same header through g++ and glibc): NOT byte-equal, and not required to be: the device's
log, acos, sin, cos and exp are not glibc's, and one ulp in an error entry is 1e-7 in a numeric Jacobian.  It is held to the same
16 D, and the test prints how many scenes happen to be byte-equal.  Measured on an MI355X: DESIGN.md section 17."""
import os
import subprocess

import numpy as np
import pytest

import essential_graph_cases as ec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(msorb_mod, sc, **kw):
    kw.setdefault("iterations", sc["iterations"])
    return msorb_mod.essential_graph(msorb_mod.eg_vertices(*ec.vertex_records(sc)), sc["v0"], sc["v1"], sc["meas"], **kw)


def _counts(res):
    return tuple(int(res[k]) for k in ec.COUNTS)


@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    d = tmp_path_factory.mktemp("essential_graph_gpu")
    exe = str(d / "essential_graph_main")
    b = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", os.path.join(ROOT, "tests", "essential_graph_main.cc"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    scenes = [ec.scene(n) for n in ec.GPU_SCENES]
    ec.write_scenes(str(d / "in.bin"), scenes)
    p = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-2000:])
    return dict(zip(ec.GPU_SCENES, ec.read_results(str(d / "out.bin"), scenes)))


@pytest.mark.parametrize("name", ec.GPU_SCENES)
def test_against_the_restatement(msorb_mod, host_results, name):
    sc, ref, host = ec.scene(name), ec.reference(name), host_results[name]
    r = _run(msorb_mod, sc)
    again = _run(msorb_mod, sc)
    res, D, bound = r["result"], ec.golden()["D"], ec.bound()
    dd = ec.estimate_difference(r["estimates"], ref["estimates"])
    dh = ec.estimate_difference(r["estimates"], host["estimates"])
    same = r["estimates"].tobytes() == host["estimates"].tobytes()
    print(f"{name}: device / restatement {dd:.3e} = {dd / D:.4f} D, device / host program {dh:.3e} = {dh / D:.4f} D (byte-equal: {same}), "
          f"bound {bound:.3e}; counts {_counts(res)} ref {ec.counts(ref)} chi2 {res['chi2_initial']:.9e} -> {res['chi2_final']:.9e} "
          f"ref {ref['chi2_initial']:.9e} -> {ref['chi2_final']:.9e}")
    assert _counts(res) == ec.counts(ref) == ec.counts(host)
    assert dd <= bound and dh <= bound
    own = ec.scene_bound(name)   # D is set by the largest scene: each scene is also held to 16 times its own recorded spread
    assert dd <= own and dh <= own, (dd, dh, own)
    assert r["estimates"].tobytes() == again["estimates"].tobytes() and res.tobytes() == again["result"].tobytes()
    # outside the system nothing moves, bit for bit
    _, free_of, _ = ec.active_set(sc)
    out = free_of < 0
    assert r["estimates"][out].tobytes() == sc["est"][out].tobytes()
    fs = (sc["fix_scale"] != 0) & ~out
    assert r["estimates"][fs, 7].tobytes() == sc["est"][fs, 7].tobytes()


def test_the_capacity_refusal_writes_nothing(msorb_mod):
    cap = msorb_mod.essential_graph_capacity()
    assert cap == 1024
    n = cap + 2                                   # one fixed, cap + 1 free
    est = np.zeros((n, 8))
    est[:, 3] = est[:, 7] = 1.0
    est[:, 4] = np.arange(n)
    v = msorb_mod.eg_vertices(est[:, :4], est[:, 4:7], est[:, 7], (np.arange(n) == 0).astype(np.int32), 1)
    v0, v1 = np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32)
    meas = np.tile(np.array([0, 0, 0, 1, 1.0, 0, 0, 1]), (n - 1, 1))
    out = np.full((n, 8), -7.0)
    with pytest.raises(msorb_mod.MsorbError) as e:
        msorb_mod.essential_graph(v, v0, v1, meas, estimates_out=out)
    assert e.value.code == msorb_mod.E_CAPACITY
    assert (out == -7.0).all()
    # exactly at the capacity the same chain is accepted (one iteration: the solve is the 7168 x 7168 one)
    r = msorb_mod.essential_graph(v[:cap + 1], v0[:cap], v1[:cap], meas[:cap], iterations=1)
    assert int(r["result"]["iterations"]) == 1 and int(r["result"]["solver_failures"]) == 0


def test_argument_errors(msorb_mod):
    sc = ec.scene("six_free")
    v = msorb_mod.eg_vertices(*ec.vertex_records(sc))
    v0, v1 = sc["v0"], sc["v1"]
    for which, index, value in ((0, 2, len(v)), (1, 0, -1), (1, 3, int(v0[3]))):   # out of range twice, then v0 == v1
        bad = [v0.copy(), v1.copy()]
        bad[which][index] = value
        out = np.full((len(v), 8), -7.0)
        with pytest.raises(msorb_mod.MsorbError) as e:
            msorb_mod.essential_graph(v, bad[0], bad[1], sc["meas"], estimates_out=out)
        assert e.value.code == msorb_mod.E_ARG and (out == -7.0).all()


def test_no_active_edge_means_no_iteration(msorb_mod):
    sc = ec.scene("six_free")
    v = msorb_mod.eg_vertices(*ec.vertex_records(sc))
    none = np.zeros(0, np.int32)
    r = msorb_mod.essential_graph(v, none, none, np.zeros((0, 8)))
    assert _counts(r["result"]) == (0, 0, 0, 0, 0, 0) and r["estimates"].tobytes() == sc["est"].tobytes()
    allfixed = v.copy()
    allfixed["fixed"] = 1                        # every edge has two fixed ends
    r = msorb_mod.essential_graph(allfixed, sc["v0"], sc["v1"], sc["meas"])
    assert _counts(r["result"]) == (0, 0, 0, 0, 0, 0) and r["estimates"].tobytes() == sc["est"].tobytes()


def test_stage_times_in_a_process_with_the_timer_on(tmp_path):
    """MSORB_LOCAL_BA_STAGES is read once per process, so the split is taken in a child: four positive stage times after a call, and
    the solve the largest of them on 39 free vertices"""
    import sys
    script = tmp_path / "stages.py"
    script.write_text(
        "import json, sys\n"
        f"sys.path[:0] = [{os.path.join(ROOT, 'ms-slam_amd')!r}, {os.path.join(ROOT, 'tests')!r}]\n"
        "import msorb, essential_graph_cases as ec\n"
        "sc = ec.scene('chain40_loop')\n"
        "r = msorb.essential_graph(msorb.eg_vertices(*ec.vertex_records(sc)), sc['v0'], sc['v1'], sc['meas'], iterations=sc['iterations'])\n"
        "print(json.dumps(dict(stages=msorb.essential_graph_stage_ms(), trials=int(r['result']['trials']))))\n")
    env = dict(os.environ, MSORB_LOCAL_BA_STAGES="1")
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    import json
    out = json.loads(p.stdout.strip().splitlines()[-1])
    print(out)
    assert set(out["stages"]) == {"linearise", "assemble", "solve", "trial"} and out["trials"] == 3
    assert all(v > 0 for v in out["stages"].values())
    assert out["stages"]["solve"] == max(out["stages"].values())
