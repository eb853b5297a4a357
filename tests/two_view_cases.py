"""Scenes and the restatement for msorb_two_view_reconstruct (TwoViewReconstruction, src/TwoViewReconstruction.cc of the reference).

  make_scene   points seen by a pinhole camera (458 / 457 / 367 / 248 at 752 x 480) from two poses, pixel noise, gross outliers
               (uniform pixels in the second image), keypoints without a match, sets of eight drawn by the swap-with-back rule of
               :83-98 from a seeded generator
  R64          the reference's path in numpy float64 on the float inputs, written from TwoViewReconstruction.cc: Normalize,
               ComputeH21 / ComputeF21 through numpy.linalg.svd, T2.inverse() through numpy.linalg.inv, the literal scoring loops,
               the folds, the branch, ReconstructH / ReconstructF / DecomposeE, CheckRT with GeometricTools::Triangulate, sort and
               arccos.  It is not a restatement of ms-slam_amd/csrc/two_view_device.h: it shares no step with it.
  VARIANTS     R64 with one choice changed: the scores and Normalize summed right to left / pairwise; every null vector and SVD
               factor with flipped sign, and a flipped pair of singular vectors (which permutes the motion hypotheses); arccos one
               ulp off either way; and, because the code under test is float, the design matrices perturbed by 4 float ulps (the
               backward error of an orthogonal iteration in float) with the models rounded to float.
  compare      an answer (the host program's, or the mirror's) against R64.  The ORDER of the motion hypotheses depends on the signs
               an SVD hands out, so they are matched by value and every per-hypothesis quantity is compared under that permutation.

A scene is admitted when all variants agree with R64 on every decision: ok, branch, both winners, the chosen motion hypothesis,
every nGood, the winner's mask and triangulated.  Run as a script this checks admission (every named edge scene, all but one in ten
generated ones) and, given the host program of tests/two_view_main.cc as `--program PATH`, measures the largest difference between
the header's float result and R64; `--write` stores it all in tests/golden/two_view_spread.json.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "two_view_spread.json")
CAM = np.array([458.0, 457.0, 367.0, 248.0], np.float32)
WIDTH, HEIGHT = 752, 480
NO_MODEL, HOMOGRAPHY, FUNDAMENTAL = 0, 1, 2
F = np.float64
EPS32 = float(np.finfo(np.float32).eps)


# ---------------------------------------------------------------------------------------------------------------- draws

def draw_sets(seed, n, H):
    """:83-98: eight draws from the shrinking list per iteration, the drawn slot refilled with the back"""
    rng = np.random.RandomState(seed)
    sets = np.zeros((H, 8), np.int32)
    for it in range(H):
        avail = list(range(n))
        for j in range(8):
            r = int(rng.random_sample() * len(avail))
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


# --------------------------------------------------------------------------------------------------------------- scenes

def _rot(axis, angle):
    a = np.asarray(axis, F) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def _project(X):
    return np.stack([CAM[0] * X[:, 0] / X[:, 2] + CAM[2], CAM[1] * X[:, 1] / X[:, 2] + CAM[3]], 1)


def make_scene(seed, n, H, baseline=(0.3, 0.0, 0.0), angle=0.05, noise=0.5, outliers=0.1, plane=None, unmatched=(0, 0), sigma=1.0,
               h_ratio=0.5, far=0, behind=0, identical=False):
    """n matches; `plane` = tilt of z = 6 + tilt x; `far` points at 2-6 km; `behind` points behind both cameras, whose images
    satisfy the epipolar constraint; `unmatched` = keypoints without a match in frame 1 / 2"""
    rng = np.random.RandomState(seed)
    if plane is None:
        z = rng.uniform(3, 10, n)
        px = np.stack([rng.uniform(20, WIDTH - 20, n), rng.uniform(20, HEIGHT - 20, n)], 1)
        X = np.stack([(px[:, 0] - CAM[2]) / CAM[0] * z, (px[:, 1] - CAM[3]) / CAM[1] * z, z], 1)
    else:
        x, y = rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n)
        X = np.stack([x, y, 6 + plane * x], 1)
    k = 0
    for cnt, scale in ((far, rng.uniform(2000, 6000, far)), (behind, -rng.uniform(3, 8, behind))):
        X[k:k + cnt] = X[k:k + cnt] / X[k:k + cnt, 2:3] * scale[:, None]
        k += cnt
    R = _rot(rng.normal(size=3), angle) if angle else np.eye(3)
    X2 = X @ R.T + np.asarray(baseline, F)
    p1, p2 = _project(X), _project(X2)
    if identical:
        p2 = p1.copy()
    else:
        p1 = p1 + rng.normal(size=p1.shape) * noise
        p2 = p2 + rng.normal(size=p2.shape) * noise
    n_out = int(round(outliers * n))
    out = n - 1 - np.arange(n_out)                      # the last matches; `far` and `behind` are the first
    p2[out] = np.stack([rng.uniform(0, WIDTH, n_out), rng.uniform(0, HEIGHT, n_out)], 1)
    # keypoints without a match, and frame 2 in an order of its own
    u1, u2 = unmatched
    n1, n2 = n + u1, n + u2
    slot1 = np.sort(rng.permutation(n1)[:n])            # match order = ascending keypoint index in frame 1
    keys1 = np.stack([rng.uniform(0, WIDTH / 3, n1), rng.uniform(0, HEIGHT / 3, n1)], 1)   # the unmatched ones crowd a corner
    keys1[slot1] = p1
    slot2 = rng.permutation(n2)[:n]
    keys2 = np.stack([rng.uniform(0, WIDTH / 3, n2), rng.uniform(0, HEIGHT / 3, n2)], 1)
    keys2[slot2] = p2
    m12 = np.full(n1, -1, np.int32)
    m12[slot1] = slot2
    return dict(keys1=keys1.astype(np.float32), keys2=keys2.astype(np.float32), matches12=m12, sets=draw_sets(seed + 1000, n, H),
                cam=CAM.copy(), sigma=float(sigma), h_ratio=float(h_ratio), min_parallax=1.0, min_triangulated=50)


def _eight():
    sc = make_scene(3, 8, 1, noise=0.0, outliers=0.0)
    sc["sets"] = np.arange(8, dtype=np.int32).reshape(1, 8)
    return sc


def _repeated_pair():
    sc = make_scene(21, 120, 35, outliers=0.1)
    idx1 = np.nonzero(sc["matches12"] >= 0)[0]
    sc["keys1"][idx1[1]] = sc["keys1"][idx1[0]]
    sc["keys2"][sc["matches12"][idx1[1]]] = sc["keys2"][sc["matches12"][idx1[0]]]
    sc["sets"][0] = [0, 1, 5, 9, 20, 33, 47, 60]
    return sc


def _all_outliers():
    return make_scene(8, 90, 20, outliers=1.0, sigma=0.001)


GENERAL = dict(noise=0.5, outliers=0.1)
PLANE_OK = dict(plane=1.5, baseline=(0.8, 0.0, 0.0), angle=0.0, noise=0.4, outliers=0.1, h_ratio=0.40)
PLANE_SECOND = dict(plane=0.8, baseline=(0.5, 0.0, 0.3), angle=0.0, noise=0.4, outliers=0.1, h_ratio=0.40)

EDGE = {
    "n=8,set=all": _eight,
    "H=1": lambda: make_scene(30, 150, 1, **GENERAL),
    "n=63": lambda: make_scene(31, 63, 200, noise=0.3, outliers=0.0),
    "n=64": lambda: make_scene(32, 64, 200, noise=0.3, outliers=0.0),
    "n=65": lambda: make_scene(33, 65, 200, noise=0.3, outliers=0.0),
    "n=255": lambda: make_scene(34, 255, 60, **GENERAL),
    "n=256": lambda: make_scene(35, 256, 60, **GENERAL),
    "n=257": lambda: make_scene(36, 257, 60, unmatched=(40, 90), **GENERAL),
    "n=1025,H=200": lambda: make_scene(37, 1025, 200, noise=0.5, outliers=0.2, unmatched=(300, 100)),
    "accepted<51": lambda: make_scene(38, 40, 50, noise=0.3, outliers=0.0),
    "accepted==51": lambda: make_scene(39, 51, 50, noise=0.1, outliers=0.0),
    "repeated pair": _repeated_pair,
    "all outliers": _all_outliers,
    "behind and far": lambda: make_scene(41, 200, 100, noise=0.3, outliers=0.05, far=12, behind=6),
    "unmatched keypoints": lambda: make_scene(42, 120, 100, unmatched=(200, 35), **GENERAL),
    "F fails: pure rotation": lambda: make_scene(43, 300, 200, baseline=(0, 0, 0), noise=0.5, outliers=0.2),
    "F fails: n=65,40% outliers": lambda: make_scene(44, 65, 200, noise=0.5, outliers=0.4),
    "F fails: n=1025,40% outliers": lambda: make_scene(45, 1025, 100, noise=0.5, outliers=0.4),
    "H: plane": lambda: make_scene(46, 200, 200, **PLANE_OK),
    "H fails: second best": lambda: make_scene(47, 200, 200, **PLANE_SECOND),
    "H at 0.50,H=1": lambda: make_scene(5978, 200, 1, plane=1.5, baseline=(0.8, 0.0, 0.0), angle=0.0, noise=0.4, outliers=0.1),
    "H fails: identical images": lambda: make_scene(48, 100, 1, identical=True, outliers=0.0, h_ratio=0.40),
}
GENERATED = {
    f"general,n={n},seed={s}": (lambda n=n, s=s, o=o, z=z: make_scene(s, n, 200, noise=z, outliers=o))
    for n, s, o, z in ((64, 101, 0.0, 0.3), (120, 102, 0.1, 0.5), (300, 103, 0.2, 0.7), (120, 104, 0.2, 0.3), (300, 105, 0.0, 0.5),
                       (64, 106, 0.1, 0.7), (120, 107, 0.0, 0.7), (300, 108, 0.1, 0.3), (200, 109, 0.15, 0.4), (150, 110, 0.05, 0.6))
}
SCENES = dict(EDGE, **GENERATED)


# ------------------------------------------------------------------------------------------------------------- R64

class Variant:
    def __init__(self, name="R64", order=0, flip=False, flip_pair=False, acos_ulp=0, float_noise=False):
        self.name, self.order, self.flip, self.flip_pair, self.acos_ulp, self.float_noise = name, order, flip, flip_pair, acos_ulp, float_noise
        self.rng = np.random.RandomState(77)

    def sum(self, x):
        x = np.asarray(x, F).reshape(-1)
        if len(x) == 0:
            return F(0)
        if self.order == 0:
            return np.cumsum(x)[-1]                 # left to right
        if self.order == 1:
            return np.cumsum(x[::-1])[-1]
        return np.sum(x)                            # pairwise

    def null_vector(self, A):
        if self.float_noise:
            A = A * (1 + 4 * EPS32 * self.rng.uniform(-1, 1, A.shape))
        x = np.linalg.svd(A)[2][-1]
        x = -x if self.flip else x
        return x.astype(np.float32).astype(F) if self.float_noise else x

    def svd3(self, A):
        U, w, Vt = np.linalg.svd(A)
        V = Vt.T
        if self.flip:
            U, V = -U, -V
        if self.flip_pair:
            U, V = U.copy(), V.copy()
            U[:, 0], V[:, 0] = -U[:, 0], -V[:, 0]
        return U, w, V

    def acos(self, c):
        a = np.arccos(c)
        for _ in range(abs(self.acos_ulp)):
            a = np.nextafter(a, np.inf if self.acos_ulp > 0 else -np.inf)
        return a


VARIANTS = [Variant("right to left", order=1), Variant("pairwise", order=2), Variant("signs flipped", flip=True),
            Variant("pair flipped", flip_pair=True), Variant("acos +1 ulp", acos_ulp=1), Variant("acos -1 ulp", acos_ulp=-1),
            Variant("float noise", float_noise=True)]


def _normalize(keys, v):
    """:737-784 -> (normalised points, T)"""
    n = len(keys)
    mean = np.array([v.sum(keys[:, 0]), v.sum(keys[:, 1])]) / n
    c = keys - mean
    dev = np.array([v.sum(np.abs(c[:, 0])), v.sum(np.abs(c[:, 1]))]) / n
    s = 1.0 / dev
    T = np.array([[s[0], 0, -mean[0] * s[0]], [0, s[1], -mean[1] * s[1]], [0, 0, 1.0]])
    return c * s, T


def _compute_h21(p1, p2, v):
    A = np.zeros((16, 9))
    for i in range(8):
        u1, v1, u2, v2 = p1[i, 0], p1[i, 1], p2[i, 0], p2[i, 1]
        A[2 * i] = [0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2]
        A[2 * i + 1] = [u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2]
    return v.null_vector(A).reshape(3, 3)


def _compute_f21(p1, p2, v):
    A = np.zeros((8, 9))
    for i in range(8):
        u1, v1, u2, v2 = p1[i, 0], p1[i, 1], p2[i, 0], p2[i, 1]
        A[i] = [u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1]
    U, w, V = v.svd3(v.null_vector(A).reshape(3, 3))
    w = w.copy()
    w[2] = 0
    return U @ np.diag(w) @ V.T


def _score(t1, t2, v):
    """the interleaved sum of :342-390 / :418-470: a rejected term adds nothing, a NaN is added"""
    return v.sum(np.stack([t1, t2], 1))


def _check_homography(H21, H12, P1, P2, sigma, v):
    th = F(np.float32(5.991))
    inv = 1.0 / (sigma * sigma)
    u1, v1, u2, v2 = P1[:, 0], P1[:, 1], P2[:, 0], P2[:, 1]
    w = 1.0 / (H12[2, 0] * u2 + H12[2, 1] * v2 + H12[2, 2])
    a, b = (H12[0, 0] * u2 + H12[0, 1] * v2 + H12[0, 2]) * w, (H12[1, 0] * u2 + H12[1, 1] * v2 + H12[1, 2]) * w
    chi1 = ((u1 - a) ** 2 + (v1 - b) ** 2) * inv
    w = 1.0 / (H21[2, 0] * u1 + H21[2, 1] * v1 + H21[2, 2])
    a, b = (H21[0, 0] * u1 + H21[0, 1] * v1 + H21[0, 2]) * w, (H21[1, 0] * u1 + H21[1, 1] * v1 + H21[1, 2]) * w
    chi2 = ((u2 - a) ** 2 + (v2 - b) ** 2) * inv
    r1, r2 = chi1 > th, chi2 > th
    return _score(np.where(r1, 0.0, th - chi1), np.where(r2, 0.0, th - chi2), v), ~(r1 | r2), np.stack([chi1, chi2], 1)


def _check_fundamental(F21, P1, P2, sigma, v):
    th, th_score = F(np.float32(3.841)), F(np.float32(5.991))
    inv = 1.0 / (sigma * sigma)
    u1, v1, u2, v2 = P1[:, 0], P1[:, 1], P2[:, 0], P2[:, 1]
    a2, b2, c2 = (F21[r, 0] * u1 + F21[r, 1] * v1 + F21[r, 2] for r in range(3))
    num2 = a2 * u2 + b2 * v2 + c2
    chi1 = num2 * num2 / (a2 * a2 + b2 * b2) * inv
    a1, b1, c1 = (F21[0, c] * u2 + F21[1, c] * v2 + F21[2, c] for c in range(3))
    num1 = a1 * u1 + b1 * v1 + c1
    chi2 = num1 * num1 / (a1 * a1 + b1 * b1) * inv
    r1, r2 = chi1 > th, chi2 > th
    return _score(np.where(r1, 0.0, th_score - chi1), np.where(r2, 0.0, th_score - chi2), v), ~(r1 | r2), np.stack([chi1, chi2], 1)


def _inv(M):
    try:
        return np.linalg.inv(M)
    except np.linalg.LinAlgError:
        return np.full((3, 3), np.nan)


def _check_rt(R, t, P1, P2, inl, K, th2, v):
    """:786-901 -> dict(n_good, cosine, parallax, status [N] (0 rejected, 1 counted, 2 counted and vbGood), p3d [N, 3], z1, cos [N])"""
    n = len(P1)
    status, p3d, z1, cosall = np.zeros(n, np.uint8), np.zeros((n, 3)), np.full(n, np.nan), np.full(n, np.nan)
    Pa = np.hstack([K, np.zeros((3, 1))])
    Pb = K @ np.hstack([R, t.reshape(3, 1)])
    O2 = -R.T @ t
    idx = np.nonzero(inl)[0]
    if len(idx) and np.isfinite(Pb).all():
        A = np.stack([P1[idx, 0:1] * Pa[2] - Pa[0], P1[idx, 1:2] * Pa[2] - Pa[1], P2[idx, 0:1] * Pb[2] - Pb[0], P2[idx, 1:2] * Pb[2] - Pb[1]], 1)
        xh = np.linalg.svd(A)[2][:, 3, :]
        xh = -xh if v.flip else xh
        p = xh[:, :3] / xh[:, 3:4]
        fin = np.isfinite(p).all(1) & (xh[:, 3] != 0)
        d1, n2 = np.linalg.norm(p, axis=1), p - O2
        cosp = (p * n2).sum(1) / (d1 * np.linalg.norm(n2, axis=1))
        low = cosp < 0.99998
        pc2 = p @ R.T + t
        e1 = (K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2] - P1[idx, 0]) ** 2 + (K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2] - P1[idx, 1]) ** 2
        e2 = (K[0, 0] * pc2[:, 0] / pc2[:, 2] + K[0, 2] - P2[idx, 0]) ** 2 + (K[1, 1] * pc2[:, 1] / pc2[:, 2] + K[1, 2] - P2[idx, 1]) ** 2
        acc = fin & ~((p[:, 2] <= 0) & low) & ~((pc2[:, 2] <= 0) & low) & ~(e1 > th2) & ~(e2 > th2)
        status[idx] = np.where(acc, np.where(low, 2, 1), 0)
        p3d[idx[acc]] = p[acc]
        z1[idx], cosall[idx] = p[:, 2], cosp
    good = status > 0
    n_good = int(good.sum())
    cosine, parallax = 0.0, 0.0
    if n_good:
        cosine = float(np.sort(cosall[good])[min(50, n_good - 1)])
        parallax = float(v.acos(cosine) * 180 / math.pi)
    return dict(n_good=n_good, cosine=cosine, parallax=parallax, status=status, p3d=p3d, z1=z1, cos=cosall)


def _motions_f(F21, K, v):
    E = K.T @ F21 @ K
    U, _, V = v.svd3(E)
    t = U[:, 2] / np.linalg.norm(U[:, 2])
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    R1, R2 = U @ W @ V.T, U @ W.T @ V.T
    R1 = -R1 if np.linalg.det(R1) < 0 else R1
    R2 = -R2 if np.linalg.det(R2) < 0 else R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def _motions_h(H21, K, v):
    A = np.linalg.inv(K) @ H21 @ K
    U, w, V = v.svd3(A)
    Vt = V.T
    s = np.linalg.det(U) * np.linalg.det(Vt)
    d1, d2, d3 = w
    if d1 / d2 < 1.00001 or d2 / d3 < 1.00001:
        return []
    aux1, aux3 = math.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), math.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
    aux_st = math.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
    ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    st = [aux_st, -aux_st, -aux_st, aux_st]
    out = []
    for i in range(4):
        Rp = np.array([[ct, 0, -st[i]], [0, 1, 0], [st[i], 0, ct]])
        tp = np.array([x1[i], 0, -x3[i]]) * (d1 - d3)
        t = U @ tp
        out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    aux_sp = math.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
    cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
    for i in range(4):
        Rp = np.array([[cp, 0, sp[i]], [0, -1, 0], [sp[i], 0, -cp]])
        tp = np.array([x1[i], 0, x3[i]]) * (d1 + d3)
        t = U @ tp
        out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    return out


def final_f(n_good, parallax, n, min_parallax, min_triangulated):
    """:505-568 as written -> the index handed out or -1"""
    nGood1, nGood2, nGood3, nGood4 = n_good
    maxGood = max(nGood1, max(nGood2, max(nGood3, nGood4)))
    nMinGood = max(int(0.9 * n), min_triangulated)
    nsimilar = 0
    if nGood1 > 0.7 * maxGood:
        nsimilar += 1
    if nGood2 > 0.7 * maxGood:
        nsimilar += 1
    if nGood3 > 0.7 * maxGood:
        nsimilar += 1
    if nGood4 > 0.7 * maxGood:
        nsimilar += 1
    if maxGood < nMinGood or nsimilar > 1:
        return -1
    if maxGood == nGood1:
        if parallax[0] > min_parallax:
            return 0
    elif maxGood == nGood2:
        if parallax[1] > min_parallax:
            return 1
    elif maxGood == nGood3:
        if parallax[2] > min_parallax:
            return 2
    elif maxGood == nGood4:
        if parallax[3] > min_parallax:
            return 3
    return -1


def final_h(n_good, parallax, n, min_parallax, min_triangulated):
    """:693-733 as written"""
    bestGood, secondBestGood, bestSolutionIdx, bestParallax = 0, 0, -1, -1.0
    for i in range(8):
        nGood = n_good[i]
        if nGood > bestGood:
            secondBestGood = bestGood
            bestGood = nGood
            bestSolutionIdx = i
            bestParallax = parallax[i]
        elif nGood > secondBestGood:
            secondBestGood = nGood
    if secondBestGood < 0.75 * bestGood and bestParallax >= min_parallax and bestGood > min_triangulated and bestGood > 0.9 * n:
        return bestSolutionIdx
    return -1


def fold(scores):
    """:172-177 / :223-228 -> (score, winner or -1)"""
    score, winner = np.float32(0.0), -1
    for i, s in enumerate(scores):
        if s > score:
            score, winner = s, i
    return score, winner


def branch_of(SH, SF, h_ratio):
    """:113-128 on floats -> (branch, RH)"""
    SH, SF = np.float32(SH), np.float32(SF)
    if np.float32(SH + SF) == 0:
        return NO_MODEL, np.float32(0)
    RH = np.float32(SH / np.float32(SH + SF))
    return (HOMOGRAPHY if float(RH) > h_ratio else FUNDAMENTAL), RH


def matches_of(sc):
    idx1 = np.nonzero(sc["matches12"] >= 0)[0]
    return idx1, sc["matches12"][idx1]


def evaluate(sc, variant=None):
    v = variant or Variant()
    v.rng = np.random.RandomState(77)
    k1, k2 = sc["keys1"].astype(F), sc["keys2"].astype(F)
    idx1, idx2 = matches_of(sc)
    P1, P2 = k1[idx1], k2[idx2]
    n, H = len(idx1), len(sc["sets"])
    sigma = F(np.float32(sc["sigma"]))
    K = np.array([[sc["cam"][0], 0, sc["cam"][2]], [0, sc["cam"][1], sc["cam"][3]], [0, 0, 1]], F)
    with np.errstate(all="ignore"):
        pn1, T1 = _normalize(k1, v)
        pn2, T2 = _normalize(k2, v)
        scores, masks, chis, models = np.zeros((2, H)), np.zeros((2, H, n), bool), np.zeros((2, H, n, 2)), np.zeros((2, H, 3, 3))
        T2inv = _inv(T2)
        for h, st in enumerate(sc["sets"]):
            a, b = pn1[idx1[st]], pn2[idx2[st]]
            try:
                H21 = T2inv @ _compute_h21(a, b, v) @ T1
                scores[0, h], masks[0, h], chis[0, h] = _check_homography(H21, _inv(H21), P1, P2, sigma, v)
                models[0, h] = H21
            except np.linalg.LinAlgError:
                scores[0, h] = np.nan
            try:
                F21 = T2.T @ _compute_f21(a, b, v) @ T1
                scores[1, h], masks[1, h], chis[1, h] = _check_fundamental(F21, P1, P2, sigma, v)
                models[1, h] = F21
            except np.linalg.LinAlgError:
                scores[1, h] = np.nan
        SH, wh = fold(scores[0])
        SF, wf = fold(scores[1])
        out = dict(scores=scores, counts=masks.sum(2).astype(np.int32), masks=masks, chis=chis, models=models, SH=float(SH), SF=float(SF),
                   winner_h=wh, winner_f=wf, n=n)
        if SH + SF == 0:
            branch, RH = NO_MODEL, 0.0
        else:
            RH = SH / (SH + SF)
            branch = HOMOGRAPHY if RH > sc["h_ratio"] else FUNDAMENTAL
        w = wh if branch == HOMOGRAPHY else wf
        motions, inl = [], np.zeros(n, bool)
        if branch != NO_MODEL and w >= 0:
            inl = masks[branch - 1, w]
            motions = _motions_h(models[0, w], K, v) if branch == HOMOGRAPHY else _motions_f(models[1, w], K, v)
        th2 = 4.0 * float(np.float32(np.float32(sc["sigma"]) * np.float32(sc["sigma"])))
        checks = [_check_rt(R, t, P1, P2, inl, K, th2, v) for R, t in motions]
        n_inl = int(inl.sum())
        rule = final_h if branch == HOMOGRAPHY else final_f
        chosen = rule([c["n_good"] for c in checks], [c["parallax"] for c in checks], n_inl, sc["min_parallax"], sc["min_triangulated"]) if motions else -1
        n1 = len(k1)
        tri, p3d = np.zeros(n1, bool), np.zeros((n1, 3))
        if chosen >= 0:
            tri[idx1] = checks[chosen]["status"] == 2
            p3d[idx1] = checks[chosen]["p3d"]
    out.update(RH=float(RH), branch=branch, inliers=inl, n_inliers=n_inl, motions=motions, checks=checks, chosen=chosen, ok=chosen >= 0,
               triangulated=tri, p3d=p3d, T1=T1, T2=T2)
    return out


_cache = {}


def prepared(name):
    """(scene, R64 of it), computed once per process"""
    if name not in _cache:
        sc = SCENES[name]()
        _cache[name] = (sc, evaluate(sc))
    return _cache[name]


def R64(sc):
    return evaluate(sc)


# ------------------------------------------------------------------------------------------------------------- comparing

def match_motions(a, b):
    """a, b: lists of (R, t) -> perm with a[i] ~ b[perm[i]] (nearest by value), or None when that is no permutation"""
    if len(a) != len(b):
        return None
    perm = []
    for Ra, ta in a:
        d = [np.abs(np.asarray(Ra, F) - Rb).max() + np.abs(np.asarray(ta, F) - tb).max() for Rb, tb in b]
        perm.append(int(np.nanargmin(d)) if np.isfinite(d).any() else -1)
    return perm if sorted(perm) == list(range(len(b))) else None


def decisions_differ(x, ref, allow_mask=None):
    """the decisions of the admission rule, x (an evaluate() of a variant, or a program's answer as as_evaluation gives it)
    against R64 -> None or what differs.  allow_mask [n] bool: inlier bits that may differ."""
    for k in ("ok", "branch", "winner_h", "winner_f", "n_inliers"):
        if int(x[k]) != int(ref[k]) and not (k == "n_inliers" and allow_mask is not None):
            return k
    d = x["inliers"] != ref["inliers"]
    if (d & ~allow_mask).any() if allow_mask is not None else d.any():
        return f"the winner's mask ({int(d.sum())} bits)"
    perm = match_motions(x["motions"], ref["motions"])
    if perm is None:
        return "the motion hypotheses do not pair up"
    for i, p in enumerate(perm):
        if x["checks"][i]["n_good"] != ref["checks"][p]["n_good"]:
            return f"nGood of hypothesis {i}: {x['checks'][i]['n_good']} / {ref['checks'][p]['n_good']}"
    if (x["chosen"] >= 0) != (ref["chosen"] >= 0) or (x["chosen"] >= 0 and perm[x["chosen"]] != ref["chosen"]):
        return "the chosen hypothesis"
    if not np.array_equal(x["triangulated"], ref["triangulated"]):
        return "triangulated"
    return None


def result_difference(x, ref):
    """-> (largest |R - R64|, |t - t64|, |p3d - p3d64| / depth) over the paired motion hypotheses and the chosen points"""
    perm = match_motions(x["motions"], ref["motions"])
    dR = dt = dp = 0.0
    if perm:
        for (R, t), p in zip(x["motions"], perm):
            dR = max(dR, float(np.abs(np.asarray(R, F) - ref["motions"][p][0]).max()))
            dt = max(dt, float(np.abs(np.asarray(t, F) - ref["motions"][p][1]).max()))
    if ref["chosen"] >= 0 and x["chosen"] >= 0:
        both = (np.abs(ref["p3d"]).sum(1) > 0) & (np.abs(np.asarray(x["p3d"], F)).sum(1) > 0)
        if both.any():
            dp = float((np.abs(np.asarray(x["p3d"], F)[both] - ref["p3d"][both]).max(1) / np.abs(ref["p3d"][both, 2])).max())
    return dR, dt, dp


def mask_excuse(sc, ref):
    """inlier bits of the branch winner that float arithmetic may decide the other way: R64's chi-square lies closer to the
    threshold than the float rounding of that quantity.  A distance of d = sqrt(th) sigma pixels is a difference of coordinates of up
    to 752, each the result of some 8 float operations on values of that size: delta = 8 * 2^-23 * 752 = 7.2e-4 px; the chi-square
    d^2 / sigma^2 moves by 2 d delta / sigma^2."""
    n = ref["n"]
    if ref["branch"] == NO_MODEL or (ref["winner_h"] if ref["branch"] == HOMOGRAPHY else ref["winner_f"]) < 0:
        return np.zeros(n, bool)
    b = ref["branch"] - 1
    w = ref["winner_h"] if b == 0 else ref["winner_f"]
    th = float(np.float32(5.991 if b == 0 else 3.841))
    sigma = sc["sigma"]
    tol = 2 * math.sqrt(th) * sigma * (8 * EPS32 * WIDTH) / (sigma * sigma)
    return (np.abs(ref["chis"][b, w] - th) <= tol).any(1)


def admitted():
    with open(FIXTURE) as f:
        dropped = json.load(f)["not_admitted"]
    return [n for n in SCENES if n not in dropped]


def load_spread():
    with open(FIXTURE) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------- files of tests/two_view_main.cc

RESULT_DTYPE = np.dtype([("ok", "<i4"), ("branch", "<i4"), ("winner_h", "<i4"), ("winner_f", "<i4"), ("n_motion", "<i4"),
                         ("chosen", "<i4"), ("n_inliers", "<i4"), ("SH", "<f4"), ("SF", "<f4"), ("RH", "<f4"),
                         ("R", "<f4", (3, 3)), ("t", "<f4", 3), ("model", "<f4", (3, 3)), ("n_good", "<i4", 8),
                         ("parallax", "<f4", 8), ("cosine", "<f4", 8), ("motion_R", "<f4", (8, 3, 3)), ("motion_t", "<f4", (8, 3))])


def write_scenes(path, scenes):
    """int32 count, then per scene: n1, n2, H, min_triangulated (i4); cam [4], sigma, min_parallax (f4); h_ratio (f8); keys1, keys2
    (f4), matches12, sets (i4)"""
    with open(path, "wb") as f:
        f.write(np.int32(len(scenes)).tobytes())
        for sc in scenes:
            f.write(np.array([len(sc["keys1"]), len(sc["keys2"]), len(sc["sets"]), sc["min_triangulated"]], np.int32).tobytes())
            f.write(np.array(list(sc["cam"]) + [sc["sigma"], sc["min_parallax"]], np.float32).tobytes())
            f.write(np.float64(sc["h_ratio"]).tobytes())
            for k, t in (("keys1", np.float32), ("keys2", np.float32), ("matches12", np.int32), ("sets", np.int32)):
                f.write(np.ascontiguousarray(sc[k], t).tobytes())


def read_results(path, scenes):
    """per scene: result record, triangulated [n1] u1, p3d [n1, 3] f4, inliers [n] u1, scores [2, H] f4, counts [2, H] i4, masks
    [2, H, n] u1, status [8, n] u1, each block padded to 4 bytes -> dicts like the mirror's, plus status"""
    buf = open(path, "rb").read()
    out, o = [], 0

    def take(dt, count):
        nonlocal o
        a = np.frombuffer(buf, dt, count, o)
        o += a.nbytes + (-a.nbytes) % 4
        return a

    for sc in scenes:
        n1, H, n = len(sc["keys1"]), len(sc["sets"]), int((sc["matches12"] >= 0).sum())
        res = take(RESULT_DTYPE, 1)[0]
        tri = take(np.uint8, n1).astype(bool)
        p3d = take(np.float32, 3 * n1).reshape(n1, 3)
        inl = take(np.uint8, n).astype(bool)
        scores = take(np.float32, 2 * H).reshape(2, H)
        counts = take(np.int32, 2 * H).reshape(2, H)
        masks = take(np.uint8, 2 * H * n).reshape(2, H, n).astype(bool)
        status = take(np.uint8, 8 * n).reshape(8, n)
        out.append(dict(result=res, triangulated=tri, p3d=p3d, inliers=inl, scores=scores, counts=counts, masks=masks, status=status))
    assert o == len(buf), (o, len(buf))
    return out


def as_evaluation(ans):
    """an answer of the program or the mirror in the shape of evaluate()'s, for decisions_differ / result_difference"""
    r = ans["result"]
    m = int(r["n_motion"])
    return dict(ok=int(r["ok"]), branch=int(r["branch"]), winner_h=int(r["winner_h"]), winner_f=int(r["winner_f"]), n_inliers=int(r["n_inliers"]),
                inliers=ans["inliers"], motions=[(r["motion_R"][i], r["motion_t"][i]) for i in range(m)],
                checks=[dict(n_good=int(r["n_good"][i])) for i in range(m)], chosen=int(r["chosen"]), triangulated=ans["triangulated"],
                p3d=ans["p3d"])


def same_bits(a, b, keys=("triangulated", "p3d", "inliers", "scores", "counts", "masks")):
    """two answers (program / mirror) bit for bit -> None or the first thing that differs"""
    for f in RESULT_DTYPE.names:
        if np.asarray(a["result"][f]).tobytes() != np.asarray(b["result"][f]).tobytes():
            return f"result.{f}: {a['result'][f]} / {b['result'][f]}"
    for k in keys:
        if np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes():
            return k
    return None


def run_program(exe, scenes, workdir, tag="run"):
    fin, fout = os.path.join(workdir, tag + ".in"), os.path.join(workdir, tag + ".out")
    write_scenes(fin, scenes)
    p = subprocess.run([exe, "run", fin, fout], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-3000:])
    return read_results(fout, scenes)


# ------------------------------------------------------------------------------------------------------------- admission

def admit(sc, ref):
    """-> (all variants agree on every decision; the variants' largest spread on R, t, p3d / depth)"""
    agree, spread = True, [0.0, 0.0, 0.0]
    for v in VARIANTS:
        ev = evaluate(sc, v)
        why = decisions_differ(ev, ref)
        d = result_difference(ev, ref)
        print(f"    {v.name:14s} {'agrees' if why is None else 'differs: ' + why}  spread R {d[0]:.2e} t {d[1]:.2e} p3d {d[2]:.2e}", file=sys.stderr)
        agree = agree and why is None
        if why is None:
            spread = [max(a, b) for a, b in zip(spread, d)]
    return agree, spread


def _round_up(x):
    if x <= 0:
        return 0.0
    e = 10.0 ** (math.floor(math.log10(x)) - 1)
    return math.ceil(x / e) * e


if __name__ == "__main__":
    dropped, D = [], [0.0, 0.0, 0.0]
    only = [a for a in sys.argv[1:] if a in SCENES]
    for name in (only or SCENES):
        sc, ref = prepared(name)
        print(f"{name}: n={ref['n']} H={len(sc['sets'])} branch={ref['branch']} RH={ref['RH']:.3f} winners={ref['winner_h']},{ref['winner_f']} "
              f"inliers={ref['n_inliers']} nGood={[c['n_good'] for c in ref['checks']]} "
              f"parallax={[round(c['parallax'], 2) for c in ref['checks']]} chosen={ref['chosen']}", file=sys.stderr)
        ok, spread = admit(sc, ref)
        if ok:
            D = [max(a, b) for a, b in zip(D, spread)]
        else:
            dropped.append(name)
    print(f"variants' spread D = {D}; not admitted: {dropped}", file=sys.stderr)
    if only:
        sys.exit(0)
    assert not [n for n in dropped if n in EDGE], "a named edge scene is not admitted"
    assert len(dropped) * 10 <= len(GENERATED), "more than one generated scene in ten is not admitted"
    record = dict(not_admitted=dropped, variants_spread=dict(zip(("R", "t", "p3d_rel"), map(_round_up, D))))
    if "--program" in sys.argv:
        import tempfile
        exe = sys.argv[sys.argv.index("--program") + 1]
        names = [n for n in SCENES if n not in dropped]
        prep = [prepared(n) for n in names]
        worst, compared, differ, excused, gap = [0.0, 0.0, 0.0], 0, 0, 0, float("inf")
        with tempfile.TemporaryDirectory() as tmp:
            answers = run_program(exe, [sc for sc, _ in prep], tmp)
        for name, (sc, ref), ans in zip(names, prep, answers):
            x = as_evaluation(ans)
            allow = mask_excuse(sc, ref)
            why = decisions_differ(x, ref, allow)
            d = result_difference(x, ref)
            worst = [max(a, b) for a, b in zip(worst, d)]
            fin = np.isfinite(ref["scores"])
            compared += int(ref["masks"].size)
            differ += int((ans["masks"] != ref["masks"]).sum())
            excused += int((ans["inliers"] != ref["inliers"]).sum())
            for b, w in ((0, ref["winner_h"]), (1, ref["winner_f"])):
                s = np.where(fin[b], ref["scores"][b], -np.inf)
                if w >= 0 and len(s) > 1:
                    gap = min(gap, float((s[w] - np.partition(s, -2)[-2]) / s[w]))
            print(f"{name}: {'agrees' if why is None else 'DIFFERS: ' + why}  float - R64: R {d[0]:.2e} t {d[1]:.2e} p3d {d[2]:.2e}  "
                  f"hypothesis mask bits differing {int((ans['masks'] != ref['masks']).sum())}, the winner's {int((ans['inliers'] != ref['inliers']).sum())}",
                  file=sys.stderr)
        record.update(float_minus_r64=dict(zip(("R", "t", "p3d_rel"), map(_round_up, worst))), decisions_compared=compared,
                      decisions_differing=differ, winner_mask_bits_excused=excused, smallest_relative_score_gap=gap, scenes=len(names))
        print(record, file=sys.stderr)
    if "--write" in sys.argv:
        assert "--program" in sys.argv
        with open(FIXTURE, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")
