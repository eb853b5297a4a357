"""msorb_create_new_map_points_kf on the CPU: the restatements of tests/new_map_points_cases.py against each other and against
ms-slam_amd/csrc/new_points_device.h compiled for the host (tests/new_points_main.cc, plain and under the address / undefined-behaviour
sanitizers), before any GPU run.

Measured here and recorded in tests/golden/new_map_points_sensitivity.json: R32 and R64 decide every pair of the four consistent
scenes alike; their points differ by at most 2.75e-5 of the point's depth; the rational form of cos(2 atan2(mb/2, depth)) differs
from numpy's float32 cos(2 arctan2()) by at most one float ulp of 1 (5.96e-8).  The hand-built scene `degenerate` is left out of
the R64 comparison: its `x3Dh(3) == 0` and `dist == 0` are exact bit patterns of the float arithmetic, which another SVD does not
reproduce."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import new_map_points_cases as nmp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT_EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def runs(oracle):
    out = {name: (sc, nmp.R32(sc, detail=True)) for name, sc in ((n, mk()) for n, mk in nmp.SCENES.items())}
    return out


@pytest.fixture(scope="module")
def natural(runs):
    return {name: (runs[name][0], runs[name][1], nmp.R64(runs[name][0], detail=True)) for name in nmp.NATURAL}


def test_every_status_code_occurs(runs):
    seen = np.zeros(14, np.int64)
    for _, r in runs.values():
        for nb in r:
            seen += np.bincount(nb["status"], minlength=14)
            assert nb["nmatches"] == int((nb["match12"] >= 0).sum()) == int((nb["status"] != nmp.NONE).sum())
    missing = [nmp.STATUS_NAMES[c] for c in range(14) if seen[c] == 0]
    assert not missing, (missing, seen)


def test_a_freed_train_is_reclaimed(runs):
    """Scene `reclaimed`: with the masks kept stale (one batched search over all neighbours) a query that already has its point
    claims a train again at a later neighbour; in the loop it is no query there, and ANOTHER query, still without a point, takes
    that train."""
    sc, r = runs["reclaimed"]
    s = nmp.stale(sc)
    assert np.array_equal(s[0]["match12"], r[0]["match12"])          # nothing differs before the first point exists
    has_point = np.zeros(len(sc["valid1"]), bool)
    found = 0
    for k in range(len(r)):
        a, b = r[k]["match12"], s[k]["match12"]
        for i in np.nonzero((a != b) & (a >= 0) & ~has_point)[0]:
            holder = np.nonzero(b == a[i])[0]                        # who holds that train in the stale run
            found += len(holder) == 1 and bool(has_point[holder[0]])
        has_point |= (r[k]["status"] >= nmp.TRIANGULATED) & (r[k]["status"] <= nmp.STEREO2)
    assert found > 0


def test_r32_and_r64_agree_and_no_decision_is_close(natural):
    """Equal statuses and matches everywhere; x3D within the recorded D of the point's depth; no comparison of :603-711 closer to
    its threshold than 16 times the larger of float32's epsilon and the measured R32 - R64 difference of that comparison (for the
    two that read the stereo cosine: also of the two forms of that cosine)."""
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "new_map_points_sensitivity.json")))
    for name, (_, r32, r64) in natural.items():
        for k, (a, b) in enumerate(zip(r32, r64)):
            assert np.array_equal(a["match12"], b["match12"]) and np.array_equal(a["status"], b["status"]), (name, k)
    m = nmp.measure_sensitivity(natural)
    print("measured", m)
    assert m["x3d_rel_depth"] <= rec["x3d_rel_depth"]
    assert m["cos_form_vs_libm"] <= rec["cos_form_vs_libm"]
    assert set(m["comparisons"]) == set(rec["comparisons"])
    for kind, v in m["comparisons"].items():
        diff = max(v["difference"], FLOAT_EPS)
        if kind in ("parallax_vs_stereo", "stereo_order"):
            diff = max(diff, m["cos_form_vs_libm"])
        assert v["closest"] >= 16 * diff, (kind, v)
        assert v["closest"] >= rec["comparisons"][kind]["closest"] and v["difference"] <= rec["comparisons"][kind]["difference"], kind


@pytest.fixture(scope="module")
def mains(tmp_path_factory):
    d = tmp_path_factory.mktemp("new_points_main")
    src = os.path.join(ROOT, "tests", "new_points_main.cc")
    flags = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", f"-I{ROOT}/tests/hip_stub"]
    exes = {}
    for tag, extra in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[tag] = str(d / tag)
        b = subprocess.run(["g++", *flags, *extra, src, "-o", exes[tag]], capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr
    return d, exes


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_header_on_the_host_equals_r32_bit_for_bit(runs, mains, build):
    d, exes = mains
    n_pairs = 0
    for name, (sc, r) in runs.items():
        for k, nb in enumerate(r):
            idx1 = np.nonzero(nb["match12"] >= 0)[0]
            fin, fout = str(d / "in.bin"), str(d / "out.bin")
            with open(fin, "wb") as fh:
                fh.write(nmp.pairs_file(sc, k, idx1, nb["match12"][idx1]))
            p = subprocess.run([exes[build], fin, fout], capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, (name, k, p.stderr)
            raw = open(fout, "rb").read()
            m = len(idx1)
            assert len(raw) == 13 * m
            st, X = np.frombuffer(raw[:m], np.uint8), np.frombuffer(raw[m:], np.float32).reshape(m, 3)
            assert np.array_equal(st, nb["status"][idx1]), (name, k)
            assert np.array_equal(X.view(np.uint32), nb["x3D"][idx1].view(np.uint32)), (name, k)
            n_pairs += m
    assert n_pairs > 500


def test_bad_arguments_are_refused_before_a_device_is_touched(msorb_mod):
    """What can be asked without a store (a store needs a device): a null store, a null call, a negative count and a null
    neighbour array are MSORB_E_INVALID with or without a GPU.  The arguments that need a store are in the GPU tests."""
    L = msorb_mod.lib()
    vp = C.c_void_p
    L.msorb_create_new_map_points_kf.argtypes = [vp, vp, vp, C.c_int, vp]
    call = msorb_mod.NewPointsCall()
    nb = (msorb_mod.NewPointsNeighbour * 1)()
    ms = C.c_float(7)
    assert L.msorb_create_new_map_points_kf(None, C.addressof(call), C.addressof(nb), 1, C.addressof(ms)) == msorb_mod.E_INVALID
    assert ms.value == 0
    assert L.msorb_create_new_map_points_kf(None, None, None, 0, None) == msorb_mod.E_INVALID
    assert L.msorb_create_new_map_points_kf(None, C.addressof(call), C.addressof(nb), -1, None) == msorb_mod.E_INVALID
    L.msorb_create_new_map_points_stage_ms.argtypes = [vp]
    assert L.msorb_create_new_map_points_stage_ms(None) == msorb_mod.E_INVALID
    assert C.sizeof(msorb_mod.NewPointsGeometry) == 112 and C.sizeof(msorb_mod.NewPointsCall) == 144
    assert C.sizeof(msorb_mod.NewPointsNeighbour) == 208
