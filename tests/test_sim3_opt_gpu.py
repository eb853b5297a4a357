"""Optimizer::OptimizeSim3 on the device (csrc/sim3_opt.hip) through the C ABI against the float64 restatement of
tests/sim3_opt_cases.py ('forward' order = g2o's walk over its edge list, this platform's libm).

Bounds.  D and C are the largest differences the restatement's variants (three summation orders, exp / sin / cos nudged by one
ulp) make on the estimate and on a chi2 over these very scenes (committed in tests/golden/sim3_opt_sensitivity.json, re-checked
by tests/test_sim3_opt_cpu.py).  The kernel adds in one more order (thread, wavefront butterfly, wavefronts) and has a libm of its
own, so its estimate may differ from the restatement's by 16 D and a chi2 by 16 C.  Flags and counts must be equal:
test_sim3_opt_cpu.py::test_threshold_margin shows no chi2 comes within 100 C of th2.  The one-step forms (its = {1, 1, 1}) have
figures of their own in the same file."""
import ctypes as C
import json
import threading

import numpy as np
import pytest

import sim3_opt_cases as sc

pytestmark = pytest.mark.gpu

FIELDS = ("q", "t", "s", "status", "n_pairs", "n_bad", "n_in", "iterations", "rejected_trials")
ARRAYS = ("P1c", "P2c", "obs1", "obs2", "w1", "w2")


@pytest.fixture(scope="module")
def golden():
    with open(sc.GOLDEN) as f:
        return json.load(f)


def _problem(msorb_mod, s, its=sc.ITS):
    return msorb_mod.sim3_opt_problem(s["q"], s["t"], s["s"], s["cam1"], s["cam2"], s["th2"], s["fix_scale"], s["min_pairs"],
                                      len(s["w1"]), its)


def _run(msorb_mod, s, its=sc.ITS):
    res, bad, chi2 = msorb_mod.sim3_optimization_batch(_problem(msorb_mod, s, its), *[s[k] for k in ARRAYS])
    return res[0], bad, chi2


def _same(a, b):
    return all(np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes() for f in FIELDS)


def _same_arrays(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_capacity_is_what_the_scenes_assume(msorb_mod):
    assert msorb_mod.sim3_optimization_capacity() == sc.CAPACITY and sc.CAPACITY % sc.WORKGROUP == 0


CASES = [(n, False) for n in sc.GPU_SCENES] + [(n, True) for n in sc.ONE_STEP]


@pytest.mark.parametrize("name,one_step", CASES, ids=[n + ("-one_step" if o else "") for n, o in CASES])
def test_against_the_restatement(msorb_mod, golden, name, one_step):
    s, ref = sc.scene(name), sc.reference(name, one_step=one_step)
    r, bad, chi2 = _run(msorb_mod, s, (1, 1, 1) if one_step else sc.ITS)
    g = golden["one_step"] if one_step else golden
    got = sc.result_dict(r, bad, chi2)
    d = sc.estimate_difference(got, ref, s["median_depth"])
    c = sc.chi2_difference(got["chi2"], ref["chi2"], ref["th2"])
    agree = sc.variants_agree(name, one_step)
    print(f"{name} one_step={one_step}: D={d:.3e} bound={g['estimate_bound']:.3e} C={c:.3e} bound={g['chi2_bound']:.3e} "
          f"it={got['iterations']} ref={ref['iterations']} rej={got['rejected_trials']} ref={ref['rejected_trials']} variants_agree={agree} "
          f"status={got['status']} n_bad={got['n_bad']} ref={ref['n_bad']} n_in={got['n_in']} ref={ref['n_in']} "
          f"flags_differ={int(np.sum(got['bad'] != ref['bad']))}")
    assert np.array_equal(got["bad"], ref["bad"])
    assert (got["status"], got["n_pairs"], got["n_bad"], got["n_in"]) == (ref["status"], ref["n_pairs"], ref["n_bad"], ref["n_in"])
    if ref["status"] == 1:      # the reference returns before it writes g2oS12
        assert r["q"].tobytes() == s["q"].tobytes() and r["t"].tobytes() == s["t"].tobytes() and float(r["s"]) == s["s"]
    if s["fix_scale"]:
        assert float(r["s"]) == s["s"]
    assert d <= g["estimate_bound"]
    assert c <= g["chi2_bound"]
    if agree:
        assert got["iterations"] == ref["iterations"] and got["rejected_trials"] == ref["rejected_trials"]
    else:
        assert [v >= 0 for v in got["iterations"]] == [v >= 0 for v in ref["iterations"]]
    if name == "rejected_trials" and not one_step:
        assert ref["rejected_trials"][0] > 0 and got["rejected_trials"][0] > 0      # the stale-error rule is exercised


def _batch(msorb_mod, names):
    ss = [sc.scene(n) for n in names]
    probs = np.concatenate([_problem(msorb_mod, s) for s in ss])
    cat = [np.concatenate([np.asarray(s[k], np.float32).reshape(-1) for s in ss]) for k in ARRAYS]
    return ss, probs, cat


def test_batch_equals_single_calls(msorb_mod):
    """eight mixed problems, one above the capacity and one with n = 0"""
    ss, probs, cat = _batch(msorb_mod, sc.BATCH_SCENES)
    assert len(ss) == 8 and any(len(s["w1"]) > sc.CAPACITY for s in ss) and any(len(s["w1"]) == 0 for s in ss)
    res, bad, chi2 = msorb_mod.sim3_optimization_batch(probs, *cat)
    o = 0
    for k, s in enumerate(ss):
        r1, bad1, chi1 = _run(msorb_mod, s)
        n = len(s["w1"])
        assert _same(res[k], r1), sc.BATCH_SCENES[k]
        assert _same_arrays((bad[o:o + n], chi2[o:o + n]), (bad1, chi1)), sc.BATCH_SCENES[k]
        o += n


@pytest.mark.parametrize("name", ["n257", "capacity_plus_1"])
def test_two_runs_are_bit_identical(msorb_mod, name):
    s = sc.scene(name)
    a, b = _run(msorb_mod, s), _run(msorb_mod, s)
    assert _same(a[0], b[0]) and _same_arrays(a[1:], b[1:])


def test_three_threads_return_the_bits_of_the_serial_calls(msorb_mod):
    names = ("n65", "n1000", "rejected_trials")
    want = [_run(msorb_mod, sc.scene(n)) for n in names]
    got, errors = [None] * 3, []

    def work(k):
        try:
            for _ in range(3):
                got[k] = _run(msorb_mod, sc.scene(names[k]))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(3)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for k in range(3):
        assert _same(got[k][0], want[k][0]) and _same_arrays(got[k][1:], want[k][1:]), names[k]


def test_chi2_out_may_be_null(msorb_mod):
    s = sc.scene("n63")
    a = _run(msorb_mod, s)
    res, bad, chi2 = msorb_mod.sim3_optimization_batch(_problem(msorb_mod, s), *[s[k] for k in ARRAYS], chi2=False)
    assert chi2 is None and _same(res[0], a[0]) and np.array_equal(bad, a[1])


def test_invalid_arguments_leave_the_outputs_untouched(msorb_mod):
    L = msorb_mod._sim3_opt_lib()
    s = sc.scene("n10")
    n = len(s["w1"])
    arrs = [np.ascontiguousarray(s[k], np.float32).reshape(-1) for k in ARRAYS]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def call(p, off, arrays, with_bad=True, with_res=True, n_problems=1):
        res = np.full(1, 0x55, np.uint8).repeat(msorb_mod.SIM3_OPT_RESULT_DTYPE.itemsize)
        bad = np.full(n, 0x55, np.uint8)
        chi2 = np.full(2 * n, -7.0)
        rc = L.msorb_sim3_optimization_batch(0, n_problems, ptr(p) if p is not None else None, ptr(off) if off is not None else None,
                                             *[ptr(a) if a is not None else None for a in arrays], ptr(bad) if with_bad else None,
                                             ptr(chi2), ptr(res) if with_res else None, None)
        untouched = (res == 0x55).all() and (bad == 0x55).all() and (chi2 == -7.0).all()
        return rc, untouched

    good, off = _problem(msorb_mod, s), np.array([0, n], np.int32)
    assert call(good, off, arrs) == (msorb_mod.OK, False)
    assert call(good, off, arrs, n_problems=0) == (msorb_mod.OK, True)
    E = msorb_mod.E_INVALID
    assert call(None, off, arrs) == (E, True)
    assert call(good, None, arrs) == (E, True)
    assert call(good, off, arrs, with_res=False) == (E, True)
    assert call(good, off, arrs, with_bad=False) == (E, True)
    for k in range(6):
        assert call(good, off, [None if j == k else a for j, a in enumerate(arrs)]) == (E, True), ARRAYS[k]
    assert call(good, np.array([0, n - 1], np.int32), arrs) == (E, True)          # offsets that do not match
    assert call(good, np.array([1, n + 1], np.int32), arrs) == (E, True)
    p = good.copy()
    p["n"] = -1
    assert call(p, np.array([0, -1], np.int32), arrs) == (E, True)
    for k in range(3):
        p = good.copy()
        p["its"][0, k] = 0
        assert call(p, off, arrs) == (E, True), k
