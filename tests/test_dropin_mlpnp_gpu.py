"""msorb_host::MLPnPsolver (ms-slam_amd/host/MLPnPsolver_device.h) compiled against the stand-ins of tests/slam_stub
(tests/dropin_mlpnp_main.cc) and driven like Tracking::Relocalization drives the reference's solvers (Tracking.cc:3688-3715):
rounds of iterate(5, ...) over the candidates.  Per call the return value, bNoMore, nInliers, vbInliers indexed by keypoint and Tout
against a Python replay of the reference's loop (:158-263: the OR condition, the rule over the counts, the exhaustion branch) on
the same draws: both sides draw from the generator of tests/mlpnp_stub (DUtils::Random over a generator of the test's own: the
process' rand() is not the solver's alone) after the same seed, the replay in the order the class documents (all sets of a call at
once), and the replay's hypotheses are R64 of tests/mlpnp_cases.py.  Tout is compared with the narrowed R64
pose within 16 D (tests/test_mlpnp_host.py) plus one float rounding; everything else is equal."""
import os
import struct
import subprocess

import numpy as np
import pytest

import mlpnp_cases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAS, BAD = 1, 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("dropin_mlpnp") / "dropin_mlpnp"
    subprocess.check_call(["g++", "-std=c++17", "-O2", f"-I{ROOT}/tests/mlpnp_stub", f"-I{ROOT}/tests/slam_stub", f"-I{ROOT}/tests/cv_stub", f"-I{ROOT}/ms-slam_amd/host",
                           f"-I{ROOT}/include", f"{ROOT}/tests/dropin_mlpnp_main.cc", f"-L{ROOT}/ms-slam_amd", "-lmsorb",
                           f"-Wl,-rpath,{ROOT}/ms-slam_amd", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", str(out)])
    return str(out)


def _random_int(seed):
    """DUtils::Random of tests/mlpnp_stub: a 64-bit linear congruential generator, the top 31 bits scaled to the range"""
    state = [seed & 0xFFFFFFFF]

    def draw(lo, hi):
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return int(((state[0] >> 33) / 2147483648.0) * (hi - lo + 1)) + lo
    return draw


def _candidate(seed, n, outlier_frac):
    """a scene spread over a match vector with holes: entries without a map point, bad points, matches past the keypoints"""
    rng = np.random.RandomState(seed)
    sc = mc.make_scene(seed, n, 1, outlier_frac=outlier_frac)
    n_matches = n + 12
    slots = np.sort(rng.permutation(n_matches - 2)[:n])             # the last two entries lie past the keypoints (:71)
    flags = np.zeros(n_matches, np.int32)
    flags[slots] = HAS
    spare = np.setdiff1d(np.arange(n_matches - 2), slots)
    flags[spare[:3]] = HAS | BAD
    flags[-2:] = HAS
    octave = rng.randint(0, 8, n_matches).astype(np.int32)
    uv, Xw = rng.uniform(0, 300, (n_matches, 2)).astype(np.float32), rng.uniform(-3, 3, (n_matches, 3)).astype(np.float32)
    uv[slots], Xw[slots] = sc["p2d"], sc["p3d"]
    max_err = (mc.SIGMA2[octave[slots]] * np.float32(5.991)).astype(np.float32)
    return dict(n_matches=n_matches, n_keys=n_matches - 2, flags=flags, octave=octave, uv=uv, Xw=Xw, slots=slots,
                scene=dict(p2d=sc["p2d"], p3d=sc["p3d"], max_err=max_err, cam=mc.CAM))


def _run(exe, tmp_path, cands, form, helper, chunk, rounds, seed=99, fisheye=0, min_inliers=10):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<8i", form, len(cands), helper, chunk, rounds, seed, fisheye, min_inliers))
        for c in cands:
            f.write(struct.pack("<2i", c["n_matches"], c["n_keys"]) + mc.CAM.tobytes() + mc.SIGMA2.tobytes())
            for i in range(c["n_matches"]):
                f.write(struct.pack("<2i", int(c["flags"][i]), int(c["octave"][i])) + c["uv"][i].tobytes() + c["Xw"][i].tobytes())
    subprocess.check_call([exe, fin, fout], timeout=120)
    raw = open(fout, "rb").read()
    supported = list(struct.unpack_from(f"<{len(cands)}i", raw))
    off, calls = 4 * len(cands), []
    for _ in range(rounds):
        for c in cands:
            h = struct.unpack_from("<4i", raw, off)
            T = np.frombuffer(raw, np.float32, 16, off + 16).reshape(4, 4)
            vb = np.frombuffer(raw, np.uint8, c["n_matches"], off + 80).astype(bool)
            off += 80 + c["n_matches"]
            calls.append(dict(ret=bool(h[0]), bNoMore=bool(h[1]), nInliers=h[2], size=h[3], T=T, vb=vb))
    assert off == len(raw)
    return supported, calls


class Replay:
    """the reference's members and loop (:143-266) over hypotheses that are drawn a call at a time and evaluated by R64"""

    def __init__(self, cand, random_int, min_inliers):
        self.c, self.sc, self.random_int = cand, cand["scene"], random_int
        self.N = len(self.sc["p2d"])
        self.min, self.max_its = mc.ransac_parameters(self.N, 0.99, min_inliers, 300, 6, 0.5)
        self.it = self.best = 0
        self.best_h = None
        self.sets, self.ev = [], None

    def lacking(self, n_iterations):
        return max(self.max_its - self.it, n_iterations) + self.it - len(self.sets)

    def draw(self, k):
        self.sets += [mc.draw_set(self.random_int, self.N) for _ in range(k)]

    def evaluate(self):
        done = 0 if self.ev is None else len(self.ev["counts"])
        if done < len(self.sets):
            new = mc.evaluate(dict(self.sc, sets=np.array(self.sets[done:], np.int32)))
            self.ev = new if self.ev is None else {k: np.concatenate([self.ev[k], new[k]]) for k in new}

    def hand(self, h):
        vb = np.zeros(self.c["n_matches"], bool)
        vb[self.c["slots"][self.ev["masks"][h]]] = True
        return vb, self.ev["poses"][h]

    def iterate(self, n_iterations):
        out = dict(ret=False, bNoMore=False, nInliers=0, vb=np.zeros(self.c["n_matches"], bool), pose=None, size=0)
        if self.N < self.min:
            out["bNoMore"] = True
            return out
        k = self.lacking(n_iterations)
        if k > 0:
            self.draw(k)
        self.evaluate()
        cur = 0
        while self.it < self.max_its or cur < n_iterations:          # :158
            cur += 1
            self.it += 1
            h = self.it - 1
            c = int(self.ev["counts"][h])
            if c >= self.min:
                if c > self.best:
                    self.best, self.best_h = c, h
                if c > self.min:                                         # Refine(), :379
                    vb, pose = self.hand(h)
                    return dict(ret=True, bNoMore=False, nInliers=c, vb=vb, pose=pose, size=len(vb))
        if self.it >= self.max_its:
            out["bNoMore"] = True
            if self.best >= self.min and self.best_h is not None:
                vb, pose = self.hand(self.best_h)
                return dict(ret=True, bNoMore=True, nInliers=self.best, vb=vb, pose=pose, size=len(vb))
        return out


def _compare(got, want, k):
    assert (got["ret"], got["bNoMore"], got["nInliers"], got["size"]) == (want["ret"], want["bNoMore"], want["nInliers"], want["size"]), k
    assert np.array_equal(got["vb"], want["vb"]), k
    T = np.eye(4)
    if want["pose"] is not None:
        T[:3, :3], T[:3, 3] = want["pose"][:9].reshape(3, 3), want["pose"][9:]
    tol = 16 * mc.load_spread() + 2.0 ** -24 * np.maximum(np.abs(T), 1.0)
    assert (np.abs(got["T"].astype(np.float64) - T) <= tol).all(), k
    assert np.array_equal(got["T"][3], [0, 0, 0, 1])


def _drive(exe, tmp_path, cands, form, helper, chunk, rounds, min_inliers=10, seed=99):
    supported, calls = _run(exe, tmp_path, cands, form, helper, chunk, rounds, seed=seed, min_inliers=min_inliers)
    assert supported == [1] * len(cands)
    ri = _random_int(seed)
    reps = [Replay(c, ri, min_inliers) for c in cands]
    if helper:                     # EvaluateFirst: the draws of every solver's first call, solver by solver
        for r in reps:
            if r.N >= r.min:
                r.draw(r.lacking(chunk))
    want = []
    for _ in range(rounds):
        for r in reps:
            want.append(r.iterate(chunk))
    for k, (g, w) in enumerate(zip(calls, want)):
        _compare(g, w, k)
    return want, reps


@pytest.mark.parametrize("form", [0, 1])
def test_a_solver_that_converges_and_is_called_again(exe, tmp_path, form):
    want, reps = _drive(exe, tmp_path, [_candidate(201, 60, 0.3)], form, 0, 5, 8)
    assert want[0]["ret"] and not want[0]["bNoMore"] and want[0]["nInliers"] > reps[0].min
    assert 0 < reps[0].it and len(reps[0].sets) > reps[0].max_its      # the later calls ran past the first call's hypotheses
    assert any(w["bNoMore"] for w in want[1:])


def test_a_solver_that_exhausts(exe, tmp_path):
    """min_inliers above every count: nothing is handed out, and iterate(35) goes 35 iterations although mRansacMaxIts is 2 (the OR
    of :158).  Then min_inliers at the largest of those counts: that hypothesis raises the best without converging and is handed
    out at exhaustion; the call after it runs past the cache."""
    cand = _candidate(202, 60, 0.2)
    want, reps = _drive(exe, tmp_path, [cand], 0, 0, 35, 1, min_inliers=58)
    assert not want[0]["ret"] and want[0]["bNoMore"] and reps[0].it == 35 and reps[0].max_its == 2
    counts = reps[0].ev["counts"][:35]
    top, first = int(counts.max()), int(np.argmax(counts))
    assert top >= 30                                           # so that SetRansacParameters leaves min_inliers at it
    want, reps = _drive(exe, tmp_path, [cand], 0, 0, max(5, first + 1), 2, min_inliers=top)
    assert reps[0].min == top and reps[0].max_its <= 35
    assert want[0]["ret"] and want[0]["bNoMore"] and want[0]["nInliers"] == top and reps[0].best_h == first
    assert len(reps[0].sets) > max(reps[0].max_its, first + 1)


def test_several_solvers_evaluated_in_one_call(exe, tmp_path):
    cands = [_candidate(203, 50, 0.3), _candidate(204, 150, 0.4), _candidate(205, 8, 0.0), _candidate(206, 30, 0.9)]
    want, reps = _drive(exe, tmp_path, cands, 0, 1, 5, 3)
    assert reps[2].N < reps[2].min and want[2]["bNoMore"] and not want[2]["ret"]      # too few correspondences: never evaluated
    assert sum(w["ret"] for w in want[:4]) >= 2
    _drive(exe, tmp_path, cands, 0, 0, 5, 3)         # without the helper the draws of the solvers interleave call by call


def test_a_camera_that_is_not_a_pinhole_is_left_to_the_caller(exe, tmp_path):
    supported, calls = _run(exe, tmp_path, [_candidate(207, 40, 0.2)], 0, 1, 5, 1, fisheye=1)
    assert supported == [0] and len(calls) == 1
    c = calls[0]
    assert not c["ret"] and c["bNoMore"] and c["nInliers"] == 0 and c["size"] == 0 and not c["vb"].any()
    assert np.array_equal(c["T"], np.eye(4, dtype=np.float32))
