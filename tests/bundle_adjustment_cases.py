"""Optimizer::BundleAdjustment (src/Optimizer.cc:60-364, the body of GlobalBundleAdjustemnt; pinhole KeyFrames without a second
camera) restated in float64 numpy on the pieces of tests/local_ba_cases.py, which are imported unchanged: the edges, the plan, the
ordered sums, the Levenberg loop (levenberg), the L D L^T, the scene generator, the SE3 pieces.  Also the named scenes of the GPU tests.  No GPU, no library.

`python tests/bundle_adjustment_cases.py --measure` writes tests/golden/bundle_adjustment_sensitivity.json.

What differs from local_ba_cases.local_ba restates the reference:
  * bRobust is a switch: off, rho = chi2 and the weight is 1 (:174, :206);
  * optimize(nIterations) runs once, the count is the caller's (:269), nothing is classified;
  * no early return without a fixed KeyFrame (fixed marks mnId == GetInitKFid(), :122);
  * a stop flag that is set on entry makes optimize() return after zero iterations: the estimates are the (normalised) inputs;
  * the mono Huber width is (float)sqrt(5.99) (:128), not (float)sqrt(5.991);
  * a point without an edge is no vertex (:261-263): it is taken out before the problem is built, its output repeats its input.

`variant`: forward (g2o's order, THE REFERENCE VALUE), reverse, pairwise (the order of every sum over edges), lapack (forward sums,
the reduced system through numpy.linalg.solve, which pivots) and dense (forward sums, no Schur complement; only for scenes of at
most DENSE_MAX_KF free KeyFrames: its pure-Python factorisation of 3 P + 6 Kf unknowns is minutes beyond)."""
import json
import math
import os
import sys
import time

import numpy as np

import local_ba_cases as lc
import pose_opt_cases as pc
from local_ba_cases import Problem, ldlt_solve, make_scene, estimate_distance, smallest_movement
from pose_opt_cases import F32, F64, rotate, normalize_rotation

VARIANTS = ("forward", "reverse", "pairwise", "lapack")
DELTA_MONO = float(F32(math.sqrt(5.99)))      # Optimizer.cc:128: thHuber2D is sqrt(5.99) in this routine, not LocalBundleAdjustment's sqrt(5.991)
DELTA_STEREO = pc.DELTA_STEREO                # :129
DENSE_MAX_KF = 40


def variants_of(s):
    free = int((~np.asarray(s["kf"]["fixed"]).astype(bool)).sum())
    return VARIANTS + (("dense",) if free <= DENSE_MAX_KF else ())


def lapack_solve(S, b, x):
    """the lower triangle of S mirrored, then numpy.linalg.solve (LU with partial pivoting).  "solver failed" is what the
    factorisation without pivoting would say: S is not positive definite (no Cholesky factor)"""
    full = np.tril(S) + np.tril(S, -1).T
    try:
        np.linalg.cholesky(full)
    except np.linalg.LinAlgError:
        return False
    x[:] = np.linalg.solve(full, b)
    return True


def bundle_adjustment(s, variant="forward", n_iterations=5, robust=True, stop=False):
    """s: a scene (kf, pos_w, edge_kf, edge_point, xy, u_right, inv_sigma2).  stop: the stop flag is set on entry.
    -> dict(status, iterations, trials, rejected_trials, n_outliers (0), kf_qt_d [K, 7], kf_qt, pos_d [P, 3], pos,
    point_included [P], chi2_initial, chi2_final, lambda_final)"""
    P_all = len(s["pos_w"])
    ep_all = np.asarray(s["edge_point"], int)
    included = np.bincount(ep_all, minlength=P_all) > 0                   # :261-263
    new_index = np.cumsum(included) - 1
    sub = dict(s, pos_w=np.asarray(s["pos_w"])[included], edge_point=new_index[ep_all])
    pr = Problem(sub)
    pr.delta = np.where(pr.stereo, DELTA_STEREO, DELTA_MONO)              # :128-129, :177, :209
    kf = s["kf"]
    q_in, t_in = np.asarray(kf["q"]), np.asarray(kf["t"])
    res = dict(status=0, n_outliers=0)

    def huber(chi2):
        return pr.huber(chi2) if robust else (chi2, np.ones_like(chi2))    # :174, :206

    q = np.array([normalize_rotation(v) for v in q_in.astype(F64)]).reshape(-1, 4)      # :138 (SE3Quat's constructor normalises)
    t = t_in.astype(F64).copy()
    X = np.asarray(sub["pos_w"]).astype(F64).copy()                       # :159
    q, t, X, lam, counts_ = lc.levenberg(pr, q, t, X, variant, n_iterations, huber, stop, lapack_solve if variant == "lapack" else ldlt_solve)
    res.update(counts_)
    qt = np.concatenate([q, t], 1)
    qt[pr.fixed] = np.concatenate([q_in, t_in], 1).astype(F64)[pr.fixed]  # a fixed KeyFrame's output repeats its input
    pos = np.asarray(s["pos_w"]).astype(F64).copy()
    pos[included] = X
    res.update(kf_qt_d=qt, pos_d=pos, point_included=included, lambda_final=lam)
    res["kf_qt"], res["pos"] = qt.astype(F32), pos.astype(F32)             # :284-288, :356-362
    return res


# ---------------------------------------------------------------------------------------------------------------- scenes
def make_windowed_scene(seed, free, points, degree=6, window=8, loop_points=0, stereo=0.6, outliers=0.0, noise=1.0, rot_deg=1.0,
                        trans=0.1, point_err=0.03):
    """free KeyFrames after ONE fixed one (index 0: the InitKFid KeyFrame), poses and cameras as local_ba_cases.make_scene makes
    them.  Point p is seen by `degree` KeyFrames of a window of `window` consecutive ones whose start moves evenly from the first
    KeyFrame to the last, so the reduced system is block-banded; the `loop_points` points after them are seen by three of the
    first six and three of the last six KeyFrames (a closed loop: blocks far from the diagonal).  -> the dict of make_scene"""
    rng = np.random.default_rng(seed)
    cam = {k: float(F32(v)) for k, v in pc.KITTI.items()}
    K, P = free + 1, points + loop_points
    q_true = np.array([pc._quat_from_axis_angle(rng.normal(size=3), math.radians(rng.uniform(0, 8))) for _ in range(K)])
    t_true = rng.uniform(-1, 1, (K, 3)) * np.array([2.0, 0.5, 2.0])
    u, v, z = rng.uniform(130, 1200, P), rng.uniform(5, 370, P), rng.uniform(6, 40, P)
    X_true = np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], -1)
    is_fixed = np.zeros(K, bool)
    is_fixed[0] = True
    ek, ep = [], []
    for p in range(P):
        if p < points:
            start = (p * (K - window + 1)) // points
            ks = start + rng.choice(window, degree, replace=False)
        else:
            ks = np.concatenate([rng.choice(6, 3, replace=False), K - 6 + rng.choice(6, 3, replace=False)])
        ks = rng.permutation(ks)
        ek += list(ks)
        ep += [p] * len(ks)
    ek, ep = np.array(ek, np.int32), np.array(ep, np.int32)
    E = len(ek)
    Xc = rotate((q_true[ek, 0], q_true[ek, 1], q_true[ek, 2], q_true[ek, 3]), X_true[ep]) + t_true[ek]
    pu, pv = cam["fx"] * Xc[:, 0] / Xc[:, 2] + cam["cx"], cam["fy"] * Xc[:, 1] / Xc[:, 2] + cam["cy"]
    sigma = 1.2 ** rng.integers(0, 8, E)
    inv_sigma2 = (1.0 / (sigma * sigma)).astype(F32)
    is_stereo = rng.uniform(size=E) < stereo
    xy = np.stack([pu, pv], -1) + rng.normal(size=(E, 2)) * (noise * sigma)[:, None]
    ur = pu - cam["mbf"] / Xc[:, 2] + rng.normal(size=E) * noise * sigma
    planted = rng.uniform(size=E) < outliers
    ang, mag = rng.uniform(0, 2 * math.pi, E), rng.uniform(20, 200, E)
    xy[planted] += (np.stack([np.cos(ang), np.sin(ang)], -1) * mag[:, None])[planted]
    ur = np.where(is_stereo, ur, -1.0)
    q0, t0 = q_true.copy(), t_true.copy()
    for k in range(1, K):
        dq = pc._quat_from_axis_angle(rng.normal(size=3), math.radians(rot_deg))
        dt = rng.normal(size=3)
        q0[k] = pc._quat_mul(dq, q_true[k])
        t0[k] = rotate(dq, t_true[k]) + dt / np.linalg.norm(dt) * trans
    q0 /= np.linalg.norm(q0, axis=1)[:, None]
    X0 = X_true + rng.normal(size=(P, 3)) * (point_err * z)[:, None]
    kf = np.zeros(K, lc.KF_DTYPE)
    kf["q"], kf["t"], kf["fixed"] = q0, t0, is_fixed
    for k in cam:
        kf[k] = cam[k]
    return dict(kf=kf, pos_w=X0.astype(F32), edge_kf=ek, edge_point=ep, xy=xy.astype(F32), u_right=ur.astype(F32),
                inv_sigma2=inv_sigma2, q_true=q_true, t_true=t_true, X_true=X_true, planted=planted, median_depth=float(np.median(z)),
                depth=z)


def _without_edges_of(s, points):
    keep = ~np.isin(s["edge_point"], points)
    out = dict(s)
    for k in ("edge_kf", "edge_point", "xy", "u_right", "inv_sigma2", "planted"):
        out[k] = s[k][keep]
    return out


def _without_mono_edges(s):
    keep = np.asarray(s["u_right"]) >= 0
    out = dict(s)
    for k in ("edge_kf", "edge_point", "xy", "u_right", "inv_sigma2", "planted"):
        out[k] = s[k][keep]
    return out


_NOT_ROBUST = dict(seed=32, free=8, fixed=1, points=200, outliers=0.2)
NO_EDGE_POINTS = (0, 7, 19, 20, 39)     # the first, the last, two neighbours
# name -> (maker, its arguments, n_iterations, robust, stop).  A scene that misses a condition of tests/test_bundle_adjustment_cpu.py
# is re-seeded HERE; no bound moves.
SCENES = {
    "mono_init": (make_scene, dict(seed=31, free=2, fixed=0, init_fixed=1, points=100, stereo=0.0, degree=2), 20, True, False),
    "not_robust": (make_scene, _NOT_ROBUST, 10, False, False),
    "not_robust_twin": (make_scene, _NOT_ROBUST, 10, True, False),
    "no_edge_points": (lambda **kw: _without_edges_of(make_scene(**kw), NO_EDGE_POINTS), dict(seed=33, free=4, fixed=1, points=40), 10, True, False),
    "it0_stop": (make_scene, dict(seed=34, free=3, fixed=1, points=30, degree=3), 10, True, True),
    "rejected": (make_scene, dict(seed=15, free=8, fixed=4, points=200, outliers=0.4, rot_deg=5.0, trans=0.5), 10, True, False),
    "k129_chain": (make_windowed_scene, dict(seed=36, free=129, points=400), 5, True, False),
    "k200_loop": (make_windowed_scene, dict(seed=37, free=200, points=800, loop_points=40, outliers=0.05), 10, False, False),
    # stereo edges only: the scene also goes through msorb_local_ba, and the two routines agree on stereo edges alone (the mono
    # Huber width is sqrt(5.99) here and sqrt(5.991) there; measured with 0.9 % mono edges: the two restatements 2.4e-6 apart).
    # make_scene's stereo=1.0 still leaves the edges whose right coordinate falls left of the image mono: those are dropped.
    "k24_small": (lambda **kw: _without_mono_edges(make_scene(**kw)), dict(seed=38, free=24, fixed=6, points=600, stereo=1.0), 10, True, False),
}

_scene_cache, _ref_cache = {}, {}


def scene(name):
    if name not in _scene_cache:
        maker, kw, n_it, robust, stop = SCENES[name]
        s = maker(**kw)
        s.update(n_iterations=n_it, robust=robust, stop=stop)
        _scene_cache[name] = s
    return _scene_cache[name]


def reference(name, variant="forward"):
    """the restatement's result on a named scene, computed once per process"""
    if (name, variant) not in _ref_cache:
        s = scene(name)
        _ref_cache[name, variant] = bundle_adjustment(s, variant, s["n_iterations"], s["robust"], s["stop"])
    return _ref_cache[name, variant]


def counts(r):
    return (r["status"], r["iterations"], r["trials"], r["rejected_trials"])


def included_movement(s, r):
    """local_ba_cases.smallest_movement over the free KeyFrames and the points that are vertices"""
    sub = dict(s, pos_w=np.asarray(s["pos_w"])[r["point_included"]], depth=s["depth"][r["point_included"]])
    return smallest_movement(sub, dict(kf_qt_d=r["kf_qt_d"], pos_d=r["pos_d"][r["point_included"]]))


def measure():
    """D: the largest estimate_distance between any two variants of a scene; chi2: the largest relative difference of
    chi2_initial / chi2_final between variants; per scene and overall"""
    per, D, C = {}, 0.0, 0.0
    for name in SCENES:
        s = scene(name)
        refs = [reference(name, v) for v in variants_of(s)]
        d = c = 0.0
        for a in range(len(refs)):
            for b in range(a + 1, len(refs)):
                d = max(d, *estimate_distance(s, refs[a], refs[b]))
                for k in ("chi2_initial", "chi2_final"):
                    m = max(abs(refs[a][k]), abs(refs[b][k]))
                    c = max(c, abs(refs[a][k] - refs[b][k]) / m if m else 0.0)
        per[name] = dict(D=d, chi2=c, counts=list(counts(refs[0])), variants_agree=len({counts(r) for r in refs}) == 1,
                         movement=included_movement(s, refs[0]) if refs[0]["iterations"] else None)
        D, C = max(D, d), max(C, c)
    return dict(D=D, chi2=C, bound=16 * D, scenes=per)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bundle_adjustment_sensitivity.json")

if __name__ == "__main__":
    if "--measure" in sys.argv:
        t0 = time.perf_counter()
        m = measure()
        with open(GOLDEN, "w") as f:
            json.dump(m, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps({k: m[k] for k in ("D", "chi2", "bound")}), f"{time.perf_counter() - t0:.1f} s")
        for name, v in m["scenes"].items():
            r = reference(name)
            print(f"{name:16s} D={v['D']:.2e} chi2={v['chi2']:.2e} move={v['movement']} agree={v['variants_agree']} "
                  f"counts={[counts(reference(name, x)) for x in variants_of(scene(name))]} chi2 {r['chi2_initial']:.1f}->{r['chi2_final']:.1f}")
    else:
        print(__doc__)
