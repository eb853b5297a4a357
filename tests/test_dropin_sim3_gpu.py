"""msorb_host::Sim3Solver (ms-slam_amd/host/Sim3Solver_device.h) compiled against the stand-ins of tests/slam_stub
(tests/dropin_sim3_main.cc) and driven like LoopClosing::DetectCommonRegionsFromBoW drives the reference's solver
(LoopClosing.cc:685-696): per chunk (bNoMore, bConverge, nInliers, the bits of the returned matrix), then the final vbInliers and
the getters, against the literal loop RefSolver of tests/sim3_cases.py.  Both sides draw from the C library's rand() after the same
srand(); the restatement gets the camera-frame points the C++ side computed (Rcw * Xw + tcw there is the caller's arithmetic) and
filters the matches itself."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import sim3_cases as s3

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAS1, MATCH, BAD1, BAD2, OBS1, OBS2, NO_LOOP_KF = 1, 2, 4, 8, 16, 32, 64
GOOD = HAS1 | MATCH | OBS1 | OBS2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("dropin_sim3") / "dropin_sim3"
    subprocess.check_call(["g++", "-std=c++17", "-O2", f"-I{ROOT}/tests/slam_stub", f"-I{ROOT}/tests/cv_stub", f"-I{ROOT}/ms-slam_amd/host",
                           f"-I{ROOT}/include", f"{ROOT}/tests/dropin_sim3_main.cc", f"-L{ROOT}/ms-slam_amd", "-lmsorb",
                           f"-Wl,-rpath,{ROOT}/ms-slam_amd", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", str(out)])
    return str(out)


def _libc_random_int(seed):
    libc = ctypes.CDLL(None)
    libc.srand(ctypes.c_uint(seed))
    libc.rand.restype = ctypes.c_int
    rand_max = 2147483647      # glibc's RAND_MAX, which the C++ side is compiled against
    return lambda lo, hi: int((libc.rand() / (rand_max + 1.0)) * (hi - lo + 1)) + lo


def _case(seed, n, fix_scale, outlier_frac=0.5):
    """a scene with spoiled entries mixed in: every reason of :73-91 / :156-171 to skip one"""
    rng = np.random.RandomState(seed)
    sc = s3.make_scene(seed, n, 1, outlier_frac=outlier_frac, fix_scale=fix_scale)
    spoil = [HAS1 | OBS1, MATCH | OBS2, GOOD | BAD1, GOOD | BAD2, GOOD & ~OBS1, GOOD & ~OBS2, GOOD | NO_LOOP_KF]
    flags = np.full(n, GOOD, np.int32)
    at = rng.permutation(n)[:3 * len(spoil)]
    flags[at] = np.tile(spoil, 3)
    poses = []
    for k in range(2):
        R = s3._rot(rng.normal(size=3), 0.4 * (k + 1))
        poses.append((R.astype(np.float32), rng.uniform(-1, 1, 3).astype(np.float32)))
    Xw = [((Xc.astype(np.float64) - t.astype(np.float64)) @ R.astype(np.float64)).astype(np.float32)      # R^T (Xc - t)
          for Xc, (R, t) in zip((sc["X1"], sc["X2"]), poses)]
    return dict(n=n, fix_scale=fix_scale, flags=flags, poses=poses, Xw=Xw, oct=[rng.randint(0, 8, n).astype(np.int32) for _ in range(2)],
                cams=[sc["cam1"], sc["cam2"]])


def _run(exe, tmp_path, case, form, overload, min_inliers, max_its, chunk, rig=0, seed=4242):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<8i", int(case["fix_scale"]), form, overload, min_inliers, max_its, chunk, rig, seed))
        for k in range(2):
            R, t = case["poses"][k]
            f.write(np.ascontiguousarray(R).tobytes() + t.tobytes() + case["cams"][k].tobytes() + s3.SIGMA2.tobytes())
        f.write(struct.pack("<i", case["n"]))
        for i in range(case["n"]):
            f.write(struct.pack("<3i", int(case["flags"][i]), int(case["oct"][0][i]), int(case["oct"][1][i])) + case["Xw"][0][i].tobytes() +
                    case["Xw"][1][i].tobytes())
    subprocess.check_call([exe, fin, fout], timeout=120)
    raw = open(fout, "rb").read()
    n = case["n"]
    supported, n_chunks = struct.unpack_from("<2i", raw)
    chunks, off = [], 8
    for _ in range(n_chunks):
        b = struct.unpack_from("<3i", raw, off)
        chunks.append(dict(bNoMore=bool(b[0]), bConverge=bool(b[1]), nInliers=b[2], T=np.frombuffer(raw, np.float32, 16, off + 12).reshape(4, 4)))
        off += 76
    vb = np.frombuffer(raw, np.uint8, n, off).astype(bool)
    off += n
    g = np.frombuffer(raw, np.float32, 29, off)
    off += 116
    Xc = np.frombuffer(raw, np.float32, 6 * n, off).reshape(2, n, 3)
    return supported, chunks, vb, dict(T12=g[:16].reshape(4, 4), R=g[16:25].reshape(3, 3), t=g[25:28], s=g[28]), Xc


def _expected(case, Xc, form, overload, min_inliers, max_its, chunk, seed=4242):
    f = case["flags"]
    keep = (f & HAS1 > 0) & (f & MATCH > 0) & (f & (BAD1 | BAD2) == 0) & (f & OBS1 > 0) & (f & OBS2 > 0)
    if form == 1:
        keep &= f & NO_LOOP_KF == 0
    idx = np.nonzero(keep)[0]
    sc = dict(X1=Xc[0][idx].copy(), X2=Xc[1][idx].copy(), max_err1=s3.max_error(case["oct"][0][idx]), max_err2=s3.max_error(case["oct"][1][idx]),
              cam1=case["cams"][0], cam2=case["cams"][1], fix_scale=case["fix_scale"])
    ref = s3.RefSolver(sc, idx, case["n"], _libc_random_int(seed))
    ref.SetRansacParameters(0.99, min_inliers, max_its)
    chunks = []
    while True:
        c = ref.iterate(chunk, with_converge=overload == 0)
        chunks.append(c)
        if c["bConverge"] or c["bNoMore"]:
            return chunks, ref, len(idx)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _compare(got, want_chunks, ref):
    supported, chunks, vb, getters, _ = got
    assert supported == 1 and len(chunks) == len(want_chunks)
    for k, (g, w) in enumerate(zip(chunks, want_chunks)):
        assert (g["bNoMore"], g["bConverge"], g["nInliers"]) == (w["bNoMore"], w["bConverge"], w["nInliers"]), k
        T = np.eye(4, dtype=np.float32) if w["T"] is None else w["T"]       # no hypothesis of the chunk reached the best: the identity
        assert np.array_equal(_bits(g["T"]), _bits(T)), k
    assert np.array_equal(vb, want_chunks[-1]["vbInliers"])
    if ref.mnBestInliers > 0 or any(c["T"] is not None for c in want_chunks):
        for key in ("T12", "R", "t", "s"):
            assert np.array_equal(_bits(getters[key]), _bits(ref.best[key])), key


@pytest.mark.parametrize("form,overload,fix_scale,min_inliers,chunk", [(0, 0, False, 30, 3), (1, 0, True, 30, 20), (0, 1, False, 30, 20),
                                                                        (1, 0, False, 75, 1)])
def test_chunks_equal_the_literal_loop(exe, tmp_path, form, overload, fix_scale, min_inliers, chunk):
    case = _case(100 + form + 2 * overload, 140, fix_scale)
    got = _run(exe, tmp_path, case, form, overload, min_inliers, 300, chunk)
    want, ref, n_kept = _expected(case, got[4], form, overload, min_inliers, 300, chunk)
    assert n_kept == 140 - (21 if form == 1 else 18)
    _compare(got, want, ref)
    if min_inliers == 75:      # more than the scene's inliers: the clamp leaves a few iterations and they run out
        assert not want[-1]["bConverge"] and want[-1]["bNoMore"] and len(want) == ref.mRansacMaxIts > 1
    else:
        assert want[-1]["bConverge"] and want[-1]["vbInliers"].sum() == want[-1]["nInliers"] > min_inliers
    if chunk == 3:
        assert len(want) > 1   # converged in a later chunk than the first


def test_fewer_correspondences_than_min_inliers(exe, tmp_path):
    case = _case(7, 40, False)
    supported, chunks, vb, _, _ = _run(exe, tmp_path, case, 0, 0, 200, 300, 20)
    assert supported == 1 and len(chunks) == 1 and chunks[0]["bNoMore"] and not chunks[0]["bConverge"] and chunks[0]["nInliers"] == 0
    assert np.array_equal(chunks[0]["T"], np.eye(4, dtype=np.float32)) and not vb.any()


def test_a_second_camera_is_left_to_the_caller(exe, tmp_path):
    supported, chunks, vb, _, _ = _run(exe, tmp_path, _case(8, 40, False), 0, 0, 10, 300, 20, rig=1)
    assert supported == 0 and chunks == [] and not vb.any()
