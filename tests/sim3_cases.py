"""Scenes and restatements for msorb_sim3_ransac_batch (Sim3Solver's RANSAC, src/Sim3Solver.cc:228-518 of the reference).

  make_scene   two point clouds related by a known Sim3 plus noise and gross outliers, thresholds from octaves, triples drawn by
               the reference's swap-with-back rule (:251-265) from a seeded generator
  R32          the fixed float32 steps of ms-slam_amd/csrc/sim3_device.h in numpy, all hypotheses at once: what the device must return
               bit for bit
  R64          the same statements in float64 on the float inputs, with numpy.linalg.eigh for the eigenvector, libm's atan2 and
               Rodrigues' formula for the rotation: the reference's path (:432-447)
  select       the literal loop of :344-366 over the counts
  RefSolver    the literal Sim3Solver (SetRansacParameters :202-226, both iterate overloads :228-373) over R32, drawing as it goes

`python tests/sim3_cases.py --write` measures R32 against R64 on SCENES and writes tests/golden/sim3_ransac_sensitivity.json.
"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SWEEPS = 16   # kSim3MaxSweeps
CAM1 = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)
CAM2 = np.array([707.0912, 707.0912, 601.8873, 183.1104], np.float32)
SIGMA2 = ((np.float32(1.2) ** np.arange(8)).astype(np.float32) ** 2).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- draws

def seeded_random_int(seed):
    """a stand-in for DUtils::Random::RandomInt(min, max) over a seeded generator"""
    rng = np.random.RandomState(seed)
    return lambda lo, hi: int(rng.random_sample() * (hi - lo + 1)) + lo


def draw_triple(random_int, n):
    """:251-265: three draws from the shrinking list, the drawn slot refilled with the back"""
    avail = list(range(n))
    out = []
    for _ in range(3):
        r = random_int(0, len(avail) - 1)
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


def ransac_max_its(probability, min_inliers, n, max_iterations):
    """mRansacMaxIts after SetRansacParameters (:213-223): the epsilon is a float, pow and log run in double"""
    if min_inliers == n:
        its = 1
    else:
        eps = float(np.float32(min_inliers) / np.float32(n)) if n else math.inf
        with np.errstate(all="ignore"):
            v = np.ceil(np.log(np.float64(1 - probability)) / np.log(np.float64(1) - np.float64(eps) ** 3))
        its = int(v) if np.isfinite(v) and abs(v) < 2 ** 31 else -2 ** 31   # what x86's conversion makes of NaN / inf
    return max(1, min(its, max_iterations))


# --------------------------------------------------------------------------------------------------------------- scenes

def _rot(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def max_error(octaves):
    """mvnMaxError (:99-100): 9.210 * sigma2 in double, stored in a vector<size_t> (Sim3Solver.h:85-86), compared as a float"""
    return np.floor(9.210 * SIGMA2[octaves].astype(np.float64)).astype(np.float32)


def make_scene(seed, n, H, outlier_frac=0.4, noise=0.01, fix_scale=False, min_inliers=None, best_inliers_in=0):
    rng = np.random.RandomState(seed)
    X2 = np.stack([rng.uniform(-6, 6, n), rng.uniform(-3, 3, n), rng.uniform(5, 25, n)], 1)
    s = 1.0 if fix_scale else 1.0 + 0.4 * rng.uniform(-1, 1)
    R = _rot(rng.normal(size=3), 0.35 * rng.uniform(-1, 1))
    t = np.array([0.8, -0.3, 0.5]) * rng.uniform(0.5, 1.5)
    X1 = s * X2 @ R.T + t + noise * rng.normal(size=(n, 3))
    out = rng.permutation(n)[:int(round(outlier_frac * n))]
    X1[out] = np.stack([rng.uniform(-6, 6, len(out)), rng.uniform(-3, 3, len(out)), rng.uniform(5, 25, len(out))], 1)
    ri = seeded_random_int(seed + 1000)
    triples = np.array([draw_triple(ri, n) for _ in range(H)], np.int32).reshape(H, 3)
    return dict(X1=X1.astype(np.float32), X2=X2.astype(np.float32), max_err1=max_error(rng.randint(0, 8, n)),
                max_err2=max_error(rng.randint(0, 8, n)), triples=triples, cam1=CAM1, cam2=CAM2, fix_scale=bool(fix_scale),
                min_inliers=int(min_inliers if min_inliers is not None else max(3, int(0.3 * n))), best_inliers_in=int(best_inliers_in),
                truth=dict(s=s, R=R, t=t))


def _coincident(fix_scale):
    """correspondences 0, 1, 2 are one point in both clouds, and hypothesis 0 draws exactly them"""
    sc = make_scene(71 + fix_scale, 40, 30, fix_scale=fix_scale, min_inliers=39, outlier_frac=0.3)
    for X in (sc["X1"], sc["X2"]):
        X[1] = X[0]
        X[2] = X[0]
    sc["triples"][0] = (0, 1, 2)
    return sc


def _behind():
    """correspondence 5 lands at z = -1 in camera 1 under the true transform, correspondence 6 has z == 0 in camera 1 itself"""
    sc = make_scene(81, 70, 60, outlier_frac=0.3)
    tr = sc["truth"]
    sc["X2"][5] = (tr["R"].T @ ((np.array([0.5, 0.2, -1.0]) - tr["t"]) / tr["s"])).astype(np.float32)
    sc["X1"][6] = (1.0, 1.0, 0.0)
    return sc


def _min_equals_n():
    sc = make_scene(91, 20, 1, outlier_frac=0.0, min_inliers=20)
    assert ransac_max_its(0.99, 20, 20, 300) == 1
    return sc


SCENES = {
    "n=3": lambda: make_scene(1, 3, 4, outlier_frac=0.0, min_inliers=2),
    "n=63": lambda: make_scene(2, 63, 50),
    "n=64": lambda: make_scene(3, 64, 300, fix_scale=True),
    "n=65": lambda: make_scene(4, 65, 50, outlier_frac=0.5),
    "n=255": lambda: make_scene(5, 255, 50, fix_scale=True),
    "n=256": lambda: make_scene(6, 256, 50, outlier_frac=0.6),
    "n=257": lambda: make_scene(7, 257, 300, outlier_frac=0.5),
    "n=1025": lambda: make_scene(8, 1025, 300, outlier_frac=0.5, fix_scale=True),
    "H=1": lambda: make_scene(9, 30, 1, outlier_frac=0.2),
    "min_inliers=n": _min_equals_n,
    "exhausted": lambda: make_scene(10, 100, 300, outlier_frac=0.5, min_inliers=80),
    "ties": lambda: make_scene(11, 12, 40, outlier_frac=0.0, noise=0.0, fix_scale=True, min_inliers=12),
    "best_in_reached": lambda: make_scene(12, 100, 100, outlier_frac=0.6, min_inliers=90, best_inliers_in=25),
    "best_in_unreached": lambda: make_scene(13, 50, 40, outlier_frac=0.5, min_inliers=10, best_inliers_in=51),
    "coincident_free": lambda: _coincident(False),
    "coincident_fixed": lambda: _coincident(True),
    "behind": _behind,
}
BATCH = ("n=65", "n=257", "H=1")   # three problems of different n and H


# --------------------------------------------------------------------------------------------------------- restatements

def _mx(a, b):
    """np_max: b > a ? b : a"""
    return np.where(b > a, b, a)


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def jacobi_largest_eigenvector(A):
    """sim3_largest_eigenvector for A [H, 4, 4] in A's dtype -> q [H, 4]"""
    F = A.dtype.type
    tiny, precision = F(1.17549435e-38), F(2.384185791015625e-07)
    W = A.copy()
    H = len(W)
    V = np.zeros_like(W)
    V[:, range(4), range(4)] = 1
    d = np.abs(W[:, range(4), range(4)])
    max_diag = _mx(_mx(d[:, 0], d[:, 1]), _mx(d[:, 2], d[:, 3]))
    for _ in range(MAX_SWEEPS):
        any_rot = False
        for p in range(3):
            for r in range(p + 1, 4):
                apq = W[:, p, r].copy()
                thr = _mx(np.full(H, tiny), precision * max_diag)
                rot = np.abs(apq) > thr
                if not rot.any():
                    continue
                any_rot = True
                app, aqq = W[:, p, p].copy(), W[:, r, r].copy()
                tau = (aqq - app) / (F(2) * apq)
                w = np.sqrt(tau * tau + F(1))
                t = np.where(tau >= 0, F(1) / (tau + w), F(1) / (tau - w))
                c = F(1) / np.sqrt(t * t + F(1))
                s = t * c
                tapq = t * apq
                N = W.copy()
                N[:, p, p] = app - tapq
                N[:, r, r] = aqq + tapq
                N[:, p, r] = 0
                N[:, r, p] = 0
                NV = V.copy()
                for k in range(4):
                    if k != p and k != r:
                        akp, akq = W[:, k, p], W[:, k, r]
                        N[:, k, p] = N[:, p, k] = c * akp - s * akq
                        N[:, k, r] = N[:, r, k] = s * akp + c * akq
                    vkp, vkq = V[:, k, p], V[:, k, r]
                    NV[:, k, p] = c * vkp - s * vkq
                    NV[:, k, r] = s * vkp + c * vkq
                W = np.where(rot[:, None, None], N, W)
                V = np.where(rot[:, None, None], NV, V)
                max_diag = np.where(rot, _mx(max_diag, _mx(np.abs(W[:, p, p]), np.abs(W[:, r, r]))), max_diag)
        if not any_rot:
            break
    best = np.zeros(H, np.int64)
    ev = W[:, 0, 0].copy()
    for i in range(1, 4):
        up = W[:, i, i] > ev
        ev = np.where(up, W[:, i, i], ev)
        best = np.where(up, i, best)
    return V[np.arange(H), :, best]


def rotation_of_quaternion(q):
    """sim3_rotation_of_quaternion for q [H, 4] -> R [H, 3, 3]"""
    F = q.dtype.type
    n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    w, x, y, z = (q[:, i] / n for i in range(4))
    tx, ty, tz = F(2) * x, F(2) * y, F(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = F(1)
    R = np.stack([one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
                  one - (txx + tyy)], 1)
    return R.reshape(-1, 3, 3)


def eigh_rotation(N):
    """:432-447 as the reference reaches it, in float64: the eigenvector of the largest eigenvalue, atan2, Rodrigues"""
    H = len(N)
    q = np.full((H, 4), np.nan)
    for h in range(H):
        if not np.isfinite(N[h]).all():
            continue
        if not N[h].any():
            q[h] = (1, 0, 0, 0)     # every vector is an eigenvector: the general solver returns the identity's columns
            continue
        w, v = np.linalg.eigh(N[h])
        q[h] = v[:, int(np.argmax(w))]
    vec = q[:, 1:]
    nv = np.sqrt((vec * vec).sum(1))
    ang = np.arctan2(nv, q[:, 0])
    rv = (2 * ang / (nv + 1e-12))[:, None] * vec
    th = np.sqrt((rv * rv).sum(1))
    R = np.zeros((H, 3, 3))
    for h in range(H):
        if not np.isfinite(th[h]):
            R[h] = np.nan
        elif th[h] == 0:
            R[h] = np.eye(3)
        else:
            K = np.array([[0, -rv[h, 2], rv[h, 1]], [rv[h, 2], 0, -rv[h, 0]], [-rv[h, 1], rv[h, 0], 0]])
            R[h] = np.eye(3) + math.sin(th[h]) / th[h] * K + (1 - math.cos(th[h])) / th[h] ** 2 * (K @ K)
    return R


def compute_sim3(P1, P2, fix_scale, F, reference_path=False):
    """sim3_compute for P1 / P2 [H, 3 points, 3] -> dict of s [H], R, sR, sRinv [H, 3, 3], t, tinv [H, 3]"""
    P1, P2 = P1.astype(F), P2.astype(F)
    three = F(3)
    O1 = ((P1[:, 0] + P1[:, 1]) + P1[:, 2]) / three
    O2 = ((P2[:, 0] + P2[:, 1]) + P2[:, 2]) / three
    Pr1, Pr2 = P1 - O1[:, None, :], P2 - O2[:, None, :]          # [H, point, xyz]
    M = np.empty((len(P1), 3, 3), F)
    for r in range(3):
        for c in range(3):
            M[:, r, c] = _dot3(Pr2[:, 0, r], Pr2[:, 1, r], Pr2[:, 2, r], Pr1[:, 0, c], Pr1[:, 1, c], Pr1[:, 2, c])
    m = lambda r, c: M[:, r, c]
    N11 = (m(0, 0) + m(1, 1)) + m(2, 2)
    N12, N13, N14 = m(1, 2) - m(2, 1), m(2, 0) - m(0, 2), m(0, 1) - m(1, 0)
    N22 = (m(0, 0) - m(1, 1)) - m(2, 2)
    N23, N24 = m(0, 1) + m(1, 0), m(2, 0) + m(0, 2)
    N33 = (-m(0, 0) + m(1, 1)) - m(2, 2)
    N34 = m(1, 2) + m(2, 1)
    N44 = (-m(0, 0) - m(1, 1)) + m(2, 2)
    N = np.stack([N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44], 1).reshape(-1, 4, 4)
    R = eigh_rotation(N) if reference_path else rotation_of_quaternion(jacobi_largest_eigenvector(N))
    R = R.astype(F)
    P3 = np.empty_like(Pr2)
    for i in range(3):
        for r in range(3):
            P3[:, i, r] = _dot3(R[:, r, 0], R[:, r, 1], R[:, r, 2], Pr2[:, i, 0], Pr2[:, i, 1], Pr2[:, i, 2])
    if not fix_scale:
        a, b = (Pr1 * P3).reshape(-1, 9), (P3 * P3).reshape(-1, 9)
        nom, den = a[:, 0], b[:, 0]
        for k in range(1, 9):
            nom, den = nom + a[:, k], den + b[:, k]
        s = (nom.astype(np.float64) / den.astype(np.float64)).astype(F)
    else:
        s = np.ones(len(P1), F)
    sR = s[:, None, None] * R
    t = np.stack([O1[:, r] - _dot3(sR[:, r, 0], sR[:, r, 1], sR[:, r, 2], O2[:, 0], O2[:, 1], O2[:, 2]) for r in range(3)], 1)
    inv = (1.0 / s.astype(np.float64)).astype(F)
    sRinv = inv[:, None, None] * R.transpose(0, 2, 1)
    tinv = np.stack([-_dot3(sRinv[:, r, 0], sRinv[:, r, 1], sRinv[:, r, 2], t[:, 0], t[:, 1], t[:, 2]) for r in range(3)], 1)
    return dict(s=s, R=R, sR=sR, t=t, sRinv=sRinv, tinv=tinv)


def _project(cam, x, y, z):
    return (cam[0] * x) / z + cam[2], (cam[1] * y) / z + cam[3]


def check_inliers(T, sc, F):
    """sim3_is_inlier for every (hypothesis, correspondence) -> mask [H, n], err1, err2 [H, n]"""
    X1, X2 = sc["X1"].astype(F), sc["X2"].astype(F)
    cam1, cam2 = sc["cam1"].astype(F), sc["cam2"].astype(F)
    p1u, p1v = _project(cam1, X1[:, 0], X1[:, 1], X1[:, 2])
    p2u, p2v = _project(cam2, X2[:, 0], X2[:, 1], X2[:, 2])

    def moved(A, b, X):
        return [_dot3(A[:, r, 0, None], A[:, r, 1, None], A[:, r, 2, None], X[None, :, 0], X[None, :, 1], X[None, :, 2]) + b[:, r, None]
                for r in range(3)]
    au, av = _project(cam1, *moved(T["sR"], T["t"], X2))
    bu, bv = _project(cam2, *moved(T["sRinv"], T["tinv"], X1))
    d1u, d1v, d2u, d2v = p1u[None] - au, p1v[None] - av, bu - p2u[None], bv - p2v[None]
    err1, err2 = d1u * d1u + d1v * d1v, d2u * d2u + d2v * d2v
    return (err1 < sc["max_err1"].astype(F)[None]) & (err2 < sc["max_err2"].astype(F)[None]), err1, err2


def select(counts, min_inliers, best_in):
    """:344-366 -> (winner, converged, consumed, best)"""
    winner, best = -1, best_in
    for i, c in enumerate(counts):
        if c >= best:
            best, winner = int(c), i
            if c > min_inliers:
                return winner, 1, i + 1, best
    return winner, 0, len(counts), best


def evaluate(sc, F=np.float32, reference_path=False, detail=False):
    with np.errstate(all="ignore"):
        tr = sc["triples"]
        T = compute_sim3(sc["X1"][tr], sc["X2"][tr], sc["fix_scale"], F, reference_path)
        mask, err1, err2 = check_inliers(T, sc, F)
    counts = mask.sum(1).astype(np.int32)
    w, conv, consumed, _ = select(counts, sc["min_inliers"], sc["best_inliers_in"])
    n = len(sc["X1"])
    out = dict(counts=counts, winner=w, converged=conv, consumed=consumed, n_inliers=int(counts[w]) if w >= 0 else 0,
               inliers=mask[w].copy() if w >= 0 else np.zeros(n, bool),
               s=T["s"][w] if w >= 0 else F(0), R=T["R"][w] if w >= 0 else np.zeros((3, 3), F), t=T["t"][w] if w >= 0 else np.zeros(3, F))
    T12 = np.zeros((4, 4), F)
    if w >= 0:
        T12[:3, :3], T12[:3, 3], T12[3, 3] = T["sR"][w], T["t"][w], 1
    out["T12"] = T12
    if detail:
        out.update(mask=mask, err1=err1, err2=err2, T=T)
    return out


def R32(sc, **kw):
    return evaluate(sc, np.float32, False, **kw)


def R64(sc, **kw):
    return evaluate(sc, np.float64, True, **kw)


# ------------------------------------------------------------------------------------------------------ the device side

def problem_of(sc, **over):
    return dict({k: sc[k] for k in ("X1", "X2", "max_err1", "max_err2", "triples", "cam1", "cam2", "fix_scale", "min_inliers",
                                    "best_inliers_in")}, **over)


def _bits_equal_or_both_nonfinite(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    fin = np.isfinite(b)
    return bool(np.array_equal(np.isfinite(a), fin) and np.array_equal(a[fin].view(np.uint32), b[fin].view(np.uint32)))


def same(dev, ref):
    """None when the mirror's answer `dev` equals the restatement `ref`: integers and masks equal, floats bit-equal where the
    restatement's are finite and non-finite where they are not; otherwise the name of what differs"""
    r = dev["result"]
    if not np.array_equal(dev["counts"], ref["counts"]):
        return "counts"
    for k in ("winner", "converged", "consumed", "n_inliers"):
        if int(r[k]) != int(ref[k]):
            return k
    if not np.array_equal(dev["inliers"], ref["inliers"]):
        return "inliers"
    for k in ("s", "R", "t", "T12"):
        if not _bits_equal_or_both_nonfinite(r[k], ref[k]):
            return k
    return None


def same_bits(a, b):
    """two answers of the mirror: every byte equal"""
    return (a["result"].tobytes() == b["result"].tobytes() and np.array_equal(a["counts"], b["counts"])
            and np.array_equal(a["inliers"], b["inliers"]))


def raw_call(msorb_mod, sc, n_problems=1, n=None, n_hyp=1, triples=None, corr=None, hyp=(0, 1), null=()):
    """msorb_sim3_ransac_batch through ctypes with arguments the mirror would not let through -> (return code, outputs untouched);
    `null` names the arrays passed as NULL"""
    import ctypes as C
    L = msorb_mod.lib()
    vp = C.c_void_p
    L.msorb_sim3_ransac_batch.argtypes = [C.c_int, C.c_int] + [vp] * 12
    n_all = len(sc["X1"])
    n = n_all if n is None else n
    pr = np.zeros(1, msorb_mod.SIM3_PROBLEM_DTYPE)
    pr["n"], pr["n_hyp"], pr["min_inliers"], pr["fix_scale"] = n, n_hyp, sc["min_inliers"], sc["fix_scale"]
    pr["cam1"], pr["cam2"] = sc["cam1"], sc["cam2"]
    a = dict(problems=pr, corr=np.asarray((0, n) if corr is None else corr, np.int32), hyp=np.asarray(hyp, np.int32), X1=sc["X1"], X2=sc["X2"],
             e1=sc["max_err1"], e2=sc["max_err2"], triples=np.ascontiguousarray(sc["triples"] if triples is None else triples, np.int32),
             inl=np.full(n_all, 7, np.uint8), counts=np.full(4, 7, np.int32), res=np.full(132, 7, np.uint8), ms=np.full(1, 7, np.float32))
    ptr = [None if k in null else a[k].ctypes.data_as(vp) for k in ("problems", "corr", "hyp", "X1", "X2", "e1", "e2", "triples", "inl", "counts",
                                                                    "res", "ms")]
    rc = L.msorb_sim3_ransac_batch(0, n_problems, *ptr)
    return rc, bool((a["inl"] == 7).all() and (a["counts"] == 7).all() and (a["res"] == 7).all())


# --------------------------------------------------------------------------------------------------- the literal solver

class RefSolver:
    """Sim3Solver from its filtered arrays on: members and control flow of :202-373, one hypothesis per loop pass through R32"""

    def __init__(self, sc, indices1, mN1, random_int):
        self.sc, self.indices1, self.mN1, self.random_int = sc, list(indices1), mN1, random_int
        self.mnIterations = self.mnBestInliers = 0
        self.best = dict(T12=np.zeros((4, 4), np.float32), R=np.zeros((3, 3), np.float32), t=np.zeros(3, np.float32), s=np.float32(0))
        self.SetRansacParameters(0.99, 6, 300)

    def SetRansacParameters(self, probability, minInliers, maxIterations):
        self.N = len(self.sc["X1"])
        self.mRansacMinInliers = minInliers
        self.mRansacMaxIts = ransac_max_its(probability, minInliers, self.N, maxIterations)
        self.mnIterations = 0

    def iterate(self, nIterations, with_converge):
        """-> dict(bNoMore, bConverge, nInliers, vbInliers [mN1], T [4, 4])"""
        out = dict(bNoMore=False, bConverge=False, nInliers=0, vbInliers=np.zeros(self.mN1, bool), T=np.eye(4, dtype=np.float32))
        if self.N < self.mRansacMinInliers:
            out["bNoMore"] = True
            return out
        bestSim3 = None
        n_cur = 0
        while self.mnIterations < self.mRansacMaxIts and n_cur < nIterations:
            n_cur += 1
            self.mnIterations += 1
            one = dict(self.sc, triples=np.array([draw_triple(self.random_int, self.N)], np.int32), best_inliers_in=0, min_inliers=0)
            h = R32(one)
            if h["n_inliers"] >= self.mnBestInliers:
                self.mnBestInliers = h["n_inliers"]
                self.best = dict(T12=h["T12"], R=h["R"], t=h["t"], s=h["s"])
                if h["n_inliers"] > self.mRansacMinInliers:
                    out["nInliers"] = h["n_inliers"]
                    out["vbInliers"][np.array(self.indices1, np.int64)[h["inliers"]]] = True
                    out["bConverge"] = True
                    out["T"] = h["T12"]
                    return out
                bestSim3 = h["T12"]
        if self.mnIterations >= self.mRansacMaxIts:
            out["bNoMore"] = True
        if with_converge:
            out["T"] = bestSim3    # None: the reference returns an uninitialised matrix here; nothing can be asked of it
        return out


# ---------------------------------------------------------------------------------------------------------- sensitivity

def measure(sc):
    """R32 against R64 on one scene -> dict"""
    a, b = R32(sc, detail=True), R64(sc, detail=True)
    agree = all(a[k] == b[k] for k in ("winner", "converged", "consumed")) and bool(np.array_equal(a["inliers"], b["inliers"]))
    m = dict(agree=agree, decisions=int(a["mask"].size), decisions_differing=int((a["mask"] != b["mask"]).sum()))
    m["share_differing"] = m["decisions_differing"] / m["decisions"]
    w = b["winner"]
    if w >= 0:
        with np.errstate(all="ignore"):
            rel = np.minimum(np.abs(b["err1"][w] - sc["max_err1"]) / sc["max_err1"], np.abs(b["err2"][w] - sc["max_err2"]) / sc["max_err2"])
        rel = rel[np.isfinite(rel)]
        m["winner_closest_to_threshold"] = float(rel.min()) if len(rel) else None
        if agree and np.isfinite(b["R"]).all() and np.isfinite(a["R"]).all():
            m["R_abs"] = float(np.abs(a["R"].astype(np.float64) - b["R"]).max())
            m["t_rel"] = float(np.abs(a["t"].astype(np.float64) - b["t"]).max() / max(np.abs(b["t"]).max(), 1e-30))
            m["s_rel"] = float(abs(float(a["s"]) - float(b["s"])) / abs(float(b["s"])))
    return m


def _round_up(x):
    if x is None or x == 0:
        return x
    e = 10.0 ** (math.floor(math.log10(abs(x))) - 1)
    return math.ceil(x / e) * e


def _round_down(x):
    if x is None or x == 0:
        return x
    e = 10.0 ** (math.floor(math.log10(abs(x))) - 1)
    return math.floor(x / e) * e


FIXTURE = os.path.join(ROOT, "tests", "golden", "sim3_ransac_sensitivity.json")

if __name__ == "__main__":
    rec = {}
    for name, mk in SCENES.items():
        m = measure(mk())
        print(name, m, file=sys.stderr)
        rec[name] = dict(decisions=m["decisions"], decisions_differing=m["decisions_differing"],
                         winner_closest_to_threshold=_round_down(m.get("winner_closest_to_threshold")),
                         R_abs=_round_up(m.get("R_abs")), t_rel=_round_up(m.get("t_rel")), s_rel=_round_up(m.get("s_rel")))
        assert m["agree"], name
    if "--write" in sys.argv:
        with open(FIXTURE, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", os.path.relpath(FIXTURE, ROOT), file=sys.stderr)
