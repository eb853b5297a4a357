"""msorb_host::TwoViewReconstruction (ms-slam_amd/host/TwoViewReconstruction_device.h) compiled against the stand-ins of
tests/slam_stub / tests/cv_stub (tests/dropin_two_view_main.cc) and driven as Pinhole::ReconstructWithTwoViews drives the
reference's class, against a literal replay of Reconstruct (:41-129): the sets drawn here from the C library's rand() after
srand(0) by the swap-with-back rule of :83-98, the models and everything after them from the host program of
tests/two_view_main.cc.  Same return value, T21 and vbTriangulated; vP3D written on the fundamental branch and left as it was on
the homography branch and on `return false`; rand() consumed as the reference consumes it: one seeding with 0, 8 * mMaxIterations
draws per call."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import two_view_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("dropin_two_view")
    dropin, host = str(d / "dropin_two_view"), str(d / "two_view_main")
    subprocess.check_call(["g++", "-std=c++17", "-O2", f"-I{ROOT}/tests/two_view_stub", f"-I{ROOT}/tests/slam_stub", f"-I{ROOT}/tests/cv_stub",
                           f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include", f"{ROOT}/tests/dropin_two_view_main.cc", f"-L{ROOT}/ms-slam_amd",
                           "-lmsorb", f"-Wl,-rpath,{ROOT}/ms-slam_amd", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", dropin])
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-O2", f"{ROOT}/tests/two_view_main.cc", "-o", host, "-lpthread"])
    return dropin, host


def _replayed_sets(n, H):
    """:81-98 over the C library's generator"""
    libc = ctypes.CDLL(None)
    libc.srand(ctypes.c_uint(0))
    libc.rand.restype = ctypes.c_int
    rand_max = 2147483647      # glibc's RAND_MAX, which the C++ side is compiled against
    sets = np.zeros((H, 8), np.int32)
    for it in range(H):
        avail = list(range(n))
        for j in range(8):
            r = int((libc.rand() / (rand_max + 1.0)) * len(avail))
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


def _scene(kind):
    if kind == "fundamental":
        return tc.make_scene(201, 150, 200, noise=0.5, outliers=0.1, unmatched=(30, 10))
    if kind == "homography":          # one iteration: with 200, the best fundamental matrix fits a plane as well and RH stays below 0.50
        return tc.make_scene(6002, 200, 1, plane=1.5, baseline=(0.8, 0.0, 0.0), angle=0.0, noise=0.4, outliers=0.1)
    if kind == "fails":
        return tc.make_scene(203, 300, 200, baseline=(0, 0, 0), noise=0.5, outliers=0.2)
    sc = tc.make_scene(204, 20, 200, noise=0.1, outliers=0.0)
    sc["matches12"][np.nonzero(sc["matches12"] >= 0)[0][7:]] = -1        # 7 matches left
    return sc


def _run(exes, tmp_path, sc):
    dropin, host = exes
    n1 = len(sc["keys1"])
    fin, fout = str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")
    tc.write_scenes(fin, [sc])
    subprocess.check_call([dropin, fin, fout], timeout=120)
    raw = open(fout, "rb").read()
    ok, seedings, seed = struct.unpack_from("<3i", raw, 0)
    draws, = struct.unpack_from("<q", raw, 12)
    o = 20
    T = np.frombuffer(raw, np.float32, 12, o)
    o += 48
    tri = np.frombuffer(raw, np.uint8, n1, o)
    o += n1
    p3d = np.frombuffer(raw, np.float32, 3 * n1, o).reshape(n1, 3)
    o += 12 * n1
    win = np.frombuffer(raw, np.float32, 3 * n1, o).reshape(n1, 3)
    o += 12 * n1
    branch, ok2, seedings2 = struct.unpack_from("<3i", raw, o)
    draws2, = struct.unpack_from("<q", raw, o + 12)
    assert o + 20 == len(raw)
    return dict(ok=ok, seedings=seedings, seed=seed, draws=draws, R=T[:9].reshape(3, 3), t=T[9:], tri=tri, p3d=p3d, win=win, branch=branch,
                ok2=ok2, seedings2=seedings2, draws2=draws2)


@pytest.mark.parametrize("kind", ["fundamental", "homography", "fails"])
def test_reconstruct_equals_the_literal_replay(exes, tmp_path, kind):
    sc = _scene(kind)
    H = len(sc["sets"])
    got = _run(exes, tmp_path, sc)
    n = int((sc["matches12"] >= 0).sum())
    replay = dict(sc, sets=_replayed_sets(n, H), h_ratio=0.5)
    want = tc.run_program(exes[1], [replay], str(tmp_path))[0]
    r = want["result"]
    assert got["ok"] == int(r["ok"]) == (0 if kind == "fails" else 1)
    assert got["branch"] == int(r["branch"]) == (tc.HOMOGRAPHY if kind == "homography" else tc.FUNDAMENTAL)
    assert (got["seedings"], got["seed"], got["draws"]) == (1, 0, 8 * H)
    assert (got["seedings2"], got["draws2"]) == (1, 16 * H)
    if r["ok"]:
        assert got["R"].tobytes() == r["R"].tobytes() and got["t"].tobytes() == r["t"].tobytes()
        assert np.array_equal(got["tri"].astype(bool), want["triangulated"]) and want["triangulated"].sum() > 100
        assert got["win"].tobytes() == want["p3d"].tobytes()
        if kind == "homography":         # ReconstructH returns true without assigning vP3D (:725-731)
            assert (got["p3d"] == 7).all()
        else:
            assert got["p3d"].tobytes() == want["p3d"].tobytes()
    else:                                # nothing is written on `return false`
        assert np.array_equal(got["R"], np.eye(3, dtype=np.float32)) and not got["t"].any()
        assert (got["tri"] == 1).all() and (got["p3d"] == 7).all() and not got["win"].any()


def test_fewer_than_eight_matches_is_false_without_a_draw(exes, tmp_path):
    got = _run(exes, tmp_path, _scene("few"))
    assert (got["ok"], got["draws"], got["seedings"], got["ok2"], got["draws2"]) == (0, 0, 0, 0, 0)
    assert (got["tri"] == 1).all() and (got["p3d"] == 7).all()
