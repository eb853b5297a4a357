"""msorb_two_view_reconstruct on the device against the host program of tests/two_view_main.cc on the same scene: the same
uncontracted statements of ms-slam_amd/csrc/two_view_device.h compiled by g++ for the host, never the code under test.  The device
must equal it IN BITS: every hypothesis' score, count and mask, both winners, branch, SH, SF, RH, the model, the motion hypotheses,
every nGood, cosine and parallax, ok, R, t, triangulated, p3d.  Repeated calls give equal bits; every refused argument leaves every
output untouched and the entry still answers; h_ratio moves only the branch.  Sizes are those of the named edge scenes of
tests/two_view_cases.py (one ballot word, one pass of the workgroup, the LDS chunks), nothing above N = 1025 x 200 hypotheses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import two_view_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_answers(tmp_path_factory):
    """the host program's answer on every admitted scene, computed once"""
    d = tmp_path_factory.mktemp("two_view_gpu")
    exe = str(d / "two_view_main")
    b = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", os.path.join(ROOT, "tests", "two_view_main.cc"), "-o", exe, "-lpthread"],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    names = tc.admitted()
    scenes = [tc.SCENES[n]() for n in names]
    return dict(zip(names, zip(scenes, tc.run_program(exe, scenes, str(d)))))


def _call(msorb_mod, sc, **kw):
    return msorb_mod.two_view_reconstruct(sc["keys1"], sc["keys2"], sc["matches12"], sc["sets"], sc["cam"], sigma=sc["sigma"],
                                          h_ratio=kw.get("h_ratio", sc["h_ratio"]), min_parallax=sc["min_parallax"],
                                          min_triangulated=sc["min_triangulated"])


def test_no_named_edge_scene_is_left_out():
    assert set(tc.EDGE) <= set(tc.admitted())


@pytest.mark.parametrize("name", tc.admitted())
def test_device_equals_the_host_program_in_bits(msorb_mod, host_answers, name):
    sc, host = host_answers[name]
    dev = _call(msorb_mod, sc)
    why = tc.same_bits(dev, host)
    r = dev["result"]
    print(f"{name}: branch {r['branch']} SH {r['SH']} SF {r['SF']} winners {r['winner_h']}, {r['winner_f']} nGood {list(r['n_good'])} "
          f"chosen {r['chosen']} ok {r['ok']}: {'bit-equal' if why is None else why}")
    assert why is None, why
    assert tc.same_bits(_call(msorb_mod, sc), dev) is None          # a second call: the same bits


def test_h_ratio_moves_only_the_branch(msorb_mod, host_answers):
    sc, host = host_answers["H: plane"]
    a, b = _call(msorb_mod, sc, h_ratio=0.40), _call(msorb_mod, sc, h_ratio=0.50)
    assert a["result"]["branch"] == tc.HOMOGRAPHY and b["result"]["branch"] == tc.FUNDAMENTAL
    for k in ("scores", "counts", "masks"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("SH", "SF", "RH", "winner_h", "winner_f"):
        assert a["result"][k].tobytes() == b["result"][k].tobytes(), k
    assert a["result"]["n_motion"] == 8 and b["result"]["n_motion"] == 4


def _raw(msorb_mod, sc, null=(), **kw):
    """the entry through ctypes with arguments the mirror would not let through -> (return code, every output untouched)"""
    L = msorb_mod.lib()
    msorb_mod._two_view_argtypes(L)
    vp = C.c_void_p
    n1, n2, n = len(sc["keys1"]), len(sc["keys2"]), int((sc["matches12"] >= 0).sum())
    H = kw.get("n_hyp", len(sc["sets"]))
    a = dict(keys1=sc["keys1"], keys2=sc["keys2"], m12=np.ascontiguousarray(kw.get("m12", sc["matches12"]), np.int32),
             sets=np.ascontiguousarray(kw.get("sets", sc["sets"]), np.int32), res=np.full(604, 7, np.uint8), tri=np.full(n1, 7, np.uint8),
             p3d=np.full(3 * n1, 7, np.float32), inl=np.full(n, 7, np.uint8), scores=np.full(2 * max(H, 1), 7, np.float32),
             counts=np.full(2 * max(H, 1), 7, np.int32), masks=np.full(2 * max(H, 1) * n, 7, np.uint8), ms=np.full(1, 7, np.float32))
    p = {k: (None if k in null else v.ctypes.data_as(vp)) for k, v in a.items()}
    rc = L.msorb_two_view_reconstruct(0, kw.get("n1", n1), p["keys1"], kw.get("n2", n2), p["keys2"], p["m12"], H, p["sets"], *[float(x) for x in sc["cam"]],
                                      sc["sigma"], sc["h_ratio"], sc["min_parallax"], sc["min_triangulated"], p["res"], p["tri"], p["p3d"],
                                      p["inl"], p["scores"], p["counts"], p["masks"], p["ms"])
    return rc, all(bool((a[k] == 7).all()) for k in ("res", "tri", "p3d", "inl", "scores", "counts", "masks", "ms"))


def test_bad_arguments_are_refused_and_nothing_is_written(msorb_mod, host_answers):
    sc, host = host_answers["unmatched keypoints"]
    E = msorb_mod.E_INVALID
    n = int((sc["matches12"] >= 0).sum())
    few = sc["matches12"].copy()
    few[np.nonzero(few >= 0)[0][7:]] = -1                                # 7 matches left
    assert _raw(msorb_mod, sc, m12=few, sets=[[0, 1, 2, 3, 4, 5, 6, 0]], n_hyp=1) == (E, True)
    assert _raw(msorb_mod, sc, n_hyp=0) == (E, True)
    assert _raw(msorb_mod, sc, n_hyp=-3) == (E, True)
    one = sc["sets"][:1].copy()
    for bad in (-1, n, one[0, 2]):                                       # negative, beyond the match count, repeated within the set
        s = one.copy()
        s[0, 5] = bad
        assert _raw(msorb_mod, sc, sets=s, n_hyp=1) == (E, True), bad
    big = sc["matches12"].copy()
    big[np.nonzero(big >= 0)[0][3]] = len(sc["keys2"])                   # a match index >= n2
    assert _raw(msorb_mod, sc, m12=big) == (E, True)
    assert _raw(msorb_mod, sc, n2=int(sc["matches12"].max())) == (E, True)   # the same, by a shorter frame 2
    for k in ("keys1", "keys2", "m12", "sets", "res", "tri", "p3d", "inl"):
        assert _raw(msorb_mod, sc, null=(k,)) == (E, True), k
    assert _raw(msorb_mod, sc, n1=-1) == (E, True)
    assert _raw(msorb_mod, sc, null=("scores", "counts", "masks", "ms")) == (msorb_mod.OK, False)     # the optional outputs
    assert _raw(msorb_mod, sc) == (msorb_mod.OK, False)
    assert tc.same_bits(_call(msorb_mod, sc), host) is None              # and the entry still answers


def test_more_matches_than_the_matcher_holds_is_a_capacity_error(msorb_mod):
    n = 32769
    rng = np.random.RandomState(1)
    sc = dict(keys1=rng.uniform(0, 700, (n, 2)).astype(np.float32), keys2=rng.uniform(0, 700, (n, 2)).astype(np.float32),
              matches12=np.arange(n, dtype=np.int32), sets=np.arange(8, dtype=np.int32).reshape(1, 8), cam=tc.CAM, sigma=1.0, h_ratio=0.5,
              min_parallax=1.0, min_triangulated=50)
    assert _raw(msorb_mod, sc) == (msorb_mod.E_CAPACITY, True)
