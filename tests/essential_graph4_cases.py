"""Optimizer::OptimizeEssentialGraph4DoF (src/Optimizer.cc:5174-5458) after its gathering loops, restated in float64 numpy with
the pieces it runs: VertexPose4DoF and Edge4DoF (include/G2oTypes.h:155-189, 817-843), ImuCamPose's constructors and UpdateW
(src/G2oTypes.cc:25-71, 121-146, 222-256), ExpSO3 / LogSO3 (:777-814), NormalizeRotation (include/G2oTypes.h:68-71), g2o's numeric
Jacobian and quadratic form (core/base_binary_edge.hpp:55-90, 131-205), its Levenberg loop
(core/optimization_algorithm_levenberg.cpp:61-195) and active set (core/sparse_optimizer.cpp:234), the scene generator and the
scene list of the GPU tests.  No GPU, no library, and no code shared with ms-slam_amd/csrc/essential_graph4_device.h: the poses
are arrays, all 17 error vectors of all edges are evaluated in one pass, and the orthonormalisation is numpy.linalg.svd.

Edge4DoF has no linearizeOplus, so g2o differentiates it numerically: central differences with delta = 1e-9 through oplus.  One ulp
in an error entry is 5e-8 in a Jacobian entry, drawn again at every estimate, so two evaluations that differ only in rounding end
at poses that differ by far more than 1e-15.  `python tests/essential_graph4_cases.py --measure` measures by how much, over the
variants below, and writes tests/golden/essential_graph4_sensitivity.json.

What the restatement fixes where the reference leaves it to Eigen / libm:
  * a product of small matrices is the plain row-by-column sum, left to right, without fused multiply-adds;
  * the 4N system is solved DENSELY in the natural vertex order (the reference: a sparse Cholesky): `solver` = 'ldlt', the
    square-root-free unpivoted L D L^T that fails on a pivot !(d > 0), or 'lapack', numpy's pivoted LU;
  * `sum_order` fixes how H's blocks, b and the cost are added over the active edges: 'forward' (g2o's edge list), 'reverse',
    'pairwise' (a balanced tree);
  * `nudge` moves the results of acos, sin, cos and sqrt up by one ulp: what another libm may return;
  * `ortho` is how NormalizeRotation reaches U V^T: 'svd' (numpy.linalg.svd) or 'polar' (Newton's iteration X <- (X + X^-T) / 2
    for the polar factor, which is U V^T).
"""
import hashlib
import json
import math
import os
import sys

import numpy as np

from essential_graph_cases import ldlt_solve, ordered_sum   # the dense solve and the ordered sums are section 17's, unchanged

F64 = np.float64
DBL_MAX = sys.float_info.max
DELTA = 1e-9                       # base_binary_edge.hpp:147
SCALAR = 1.0 / (2 * DELTA)         # :148
TAU = 1e-5                         # computeLambdaInit's _tau (optimization_algorithm_levenberg.cpp:48, :185)
ITERATIONS = 20                    # optimize(20) (Optimizer.cc:5415)
OMEGA = np.array([1e3, 1e3, 1.0, 1.0, 1.0, 1.0])   # matLambda (:5240-5243): (0, 0) twice, (2, 2) never
VARIANTS = (("forward", False, "ldlt", "svd"), ("reverse", False, "ldlt", "svd"), ("pairwise", False, "ldlt", "svd"),
            ("forward", True, "ldlt", "svd"), ("forward", False, "lapack", "svd"), ("forward", False, "ldlt", "polar"))
#            (sum_order, nudge, solver, ortho); the first is THE restatement
MARGIN = 16                        # the project's margin over the measured spread (DESIGN.md sections 10, 14, 16, 17, 18)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "essential_graph4_sensitivity.json")
I3 = np.eye(3)


def _up(v, nudge):
    return np.nextafter(v, np.inf) if nudge else v


# ------------------------------------------------------------------------------------------------ small matrices over arrays
def mm(A, B):
    """[M, 3, 3] x [M, 3, 3]: the row-by-column sum, left to right"""
    return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + A[..., :, 2, None] * B[..., None, 2, :]


def mv(A, x):
    return (A[..., :, 0] * x[..., None, 0] + A[..., :, 1] * x[..., None, 1]) + A[..., :, 2] * x[..., None, 2]


def tr(A):
    return np.swapaxes(A, -1, -2)


def normalize_rotation(R, ortho="svd"):
    """NormalizeRotation (G2oTypes.h:68-71): U V^T of the SVD"""
    if ortho == "svd":
        U, _, Vt = np.linalg.svd(R)
        return mm(U, Vt)
    X = R.copy()
    for _ in range(40):
        Y = 0.5 * (X + tr(np.linalg.inv(X)))
        if np.array_equal(X, Y):
            break
        X = Y
    return X


def exp_so3(x, y, z, nudge=False, ortho="svd"):
    """ExpSO3 (G2oTypes.cc:782-798) over arrays [M] -> [M, 3, 3]"""
    x, y, z = (np.atleast_1d(np.asarray(v, F64)) for v in (x, y, z))
    d2 = (x * x + y * y) + z * z
    d = _up(np.sqrt(d2), nudge)
    o = np.zeros_like(x)
    W = np.stack([np.stack([o, -z, y], -1), np.stack([z, o, -x], -1), np.stack([-y, x, o], -1)], -2)
    small = d < 1e-5
    with np.errstate(all="ignore"):
        a = (I3 + W) + mm(0.5 * W, W)                                          # :790
        sn, cm = _up(np.sin(d), nudge), 1.0 - _up(np.cos(d), nudge)
        b = (I3 + (W * sn[:, None, None]) / d[:, None, None]) + (mm(W, W) * cm[:, None, None]) / d2[:, None, None]   # :795
    return normalize_rotation(np.where(small[:, None, None], a, b), ortho)


def log_exits(R):
    """which of LogSO3's exits each row takes: 0 costheta outside [-1, 1], 1 |sin| < 1e-5, 2 the general one"""
    c = (((R[:, 0, 0] + R[:, 1, 1]) + R[:, 2, 2]) - 1.0) * 0.5
    out = (c > 1) | (c < -1)
    with np.errstate(all="ignore"):
        s = np.sin(np.arccos(np.where(out, 0.0, c)))
    return np.where(out, 0, np.where(np.abs(s) < 1e-5, 1, 2))


def log_so3(R, nudge=False):
    """LogSO3 (G2oTypes.cc:800-814) -> [M, 3]"""
    t = (R[:, 0, 0] + R[:, 1, 1]) + R[:, 2, 2]
    w = np.stack([(R[:, 2, 1] - R[:, 1, 2]) / 2, (R[:, 0, 2] - R[:, 2, 0]) / 2, (R[:, 1, 0] - R[:, 0, 1]) / 2], 1)
    c = (t - 1.0) * 0.5
    out = (c > 1) | (c < -1)
    with np.errstate(all="ignore"):
        theta = _up(np.arccos(np.where(out, 0.0, c)), nudge)
        s = _up(np.sin(theta), nudge)
        early = out | (np.abs(s) < 1e-5)
        full = (theta[:, None] * w) / s[:, None]
    return np.where(early[:, None], w, full)


# ------------------------------------------------------------------------------------------------------------- the estimate
def initial_state(sc):
    """what either constructor leaves: DR = I, its = 0, the camera pose as handed in"""
    n = len(sc["fixed"])
    return dict(DR=np.tile(I3, (n, 1, 1)), twb=sc["twb"].copy(), Rcw=sc["Rcw"].copy(), tcw=sc["tcw"].copy(), its=np.zeros(n, int))


def camera_pose(sc, idx, DR, twb):
    """UpdateW's tail (G2oTypes.cc:231, :248-255) for the vertices idx"""
    Rwb = mm(DR, sc["Rwb"][idx])
    Rbw = tr(Rwb)
    tbw = -mv(Rbw, twb)
    return mm(sc["Rcb"][idx], Rbw), mv(sc["Rcb"][idx], tbw) + sc["tcb"][idx]


def update_w(sc, st, idx, dR, ut):
    """oplusImpl -> UpdateW({0, 0, u0, u1, u2, u3}) on the vertices idx: a new state dict (push keeps the old one)"""
    new = {k: v.copy() for k, v in st.items()}
    new["DR"][idx] = mm(dR, st["DR"][idx])                                     # :230
    new["twb"][idx] = st["twb"][idx] + ut                                      # :233
    new["Rcw"][idx], new["tcw"][idx] = camera_pose(sc, idx, new["DR"][idx], new["twb"][idx])
    its = st["its"][idx] + 1                                                   # :236-245 (NormalizeRotation(DR)'s result is dropped)
    z = idx[its >= 5]
    for r, c in ((0, 2), (1, 2), (2, 0), (2, 1)):
        new["DR"][z, r, c] = 0.0
    new["its"][idx] = np.where(its >= 5, 0, its)
    return new


def poses_of(st):
    return np.concatenate([st["Rcw"].reshape(-1, 9), st["tcw"]], 1)


def edge_errors(Ri, ti, Rj, tj, meas, nudge=False):
    """Edge4DoF::computeError (G2oTypes.h:831-836) -> [M, 6]"""
    dR, dt = meas[:, :9].reshape(-1, 3, 3), meas[:, 9:]
    rot = log_so3(mm(mm(Ri, tr(Rj)), tr(dR)), nudge)
    trans = (mv(Ri, -mv(tr(Rj), tj)) + ti) - dt
    return np.concatenate([rot, trans], 1)


def chi2_of(e):
    c = e[:, 0] * (OMEGA[0] * e[:, 0])
    for d in range(1, 6):
        c = c + e[:, d] * (OMEGA[d] * e[:, d])
    return c


def perturbation_table(nudge, ortho):
    """ExpSO3(0, 0, +delta), ExpSO3(0, 0, -delta), ExpSO3(0, 0, 0)"""
    return exp_so3([0.0] * 3, [0.0] * 3, [DELTA, -DELTA, 0.0], nudge, ortho)


# --------------------------------------------------------------------------------------------------------------- the graph
def active_set(sc):
    """(active edge indices, free_of_vertex [N] with -1 for fixed or outside the system, vertex_of_free)"""
    fixed, v0, v1 = sc["fixed"], sc["v0"], sc["v1"]
    act = [e for e in range(len(v0)) if not (fixed[v0[e]] and fixed[v1[e]])]   # sparse_optimizer.cpp:234
    used = set()
    for e in act:
        used.update(v for v in (v0[e], v1[e]) if not fixed[v])
    free_of = -np.ones(len(fixed), int)
    vof = sorted(used)
    free_of[vof] = np.arange(len(vof))
    return np.array(act, int), free_of, np.array(vof, int)


def error_vectors(sc, st, act, tab, nudge):
    """the 17 error vectors of every active edge [17, E, 6]: 0 the base error, 1 + 2 col + minus vertex 0 perturbed, 9 + ... vertex 1"""
    v0, v1 = sc["v0"][act], sc["v1"][act]
    n = len(sc["fixed"])
    allv = np.arange(n)
    R, t = np.empty((8, n, 3, 3)), np.empty((8, n, 3))
    for k in range(8):                                                         # push, oplus(+-delta e_col), pop (:157-170)
        col, step = k >> 1, (-DELTA if k & 1 else DELTA)
        dR = tab[(k & 1) if col == 0 else 2]
        add = np.zeros(3)
        if col:
            add[col - 1] = step
        R[k], t[k] = camera_pose(sc, allv, mm(dR[None], st["DR"]), st["twb"] + add)
    err = np.empty((17, len(act), 6))
    err[0] = edge_errors(st["Rcw"][v0], st["tcw"][v0], st["Rcw"][v1], st["tcw"][v1], sc["meas"][act], nudge)
    for k in range(8):
        err[1 + k] = edge_errors(R[k][v0], t[k][v0], st["Rcw"][v1], st["tcw"][v1], sc["meas"][act], nudge)
        err[9 + k] = edge_errors(st["Rcw"][v0], st["tcw"][v0], R[k][v1], t[k][v1], sc["meas"][act], nudge)
    return err


def linearise(sc, st, act, free_of, tab, order, nudge):
    """computeActiveErrors, activeRobustChi2, buildSystem -> (cost, H dense [n, n], b [n])"""
    v0, v1, E = sc["v0"][act], sc["v1"][act], len(act)
    err = error_vectors(sc, st, act, tab, nudge)
    e = err[0]
    cost = ordered_sum(chi2_of(e), order) if E else 0.0
    J = [np.stack([SCALAR * (err[1 + 8 * side + 2 * c] - err[2 + 8 * side + 2 * c]) for c in range(4)], 2) for side in (0, 1)]   # [E, d, col]

    def prod(X, Y):   # (X^T Omega) Y per edge (base_binary_edge.hpp:77-89), the sum over d left to right
        acc = (X[:, 0, :, None] * OMEGA[0]) * Y[:, 0, None, :]
        for d in range(1, 6):
            acc = acc + (X[:, d, :, None] * OMEGA[d]) * Y[:, d, None, :]
        return acc

    def upper(P):     # the solver reads the upper triangle of a diagonal block
        U = np.triu(P)
        return U + np.swapaxes(np.triu(P, 1), 1, 2)

    def rhs(X):       # X^T omega_r, omega_r = -(Omega e) (:74)
        acc = X[:, 0, :] * -(OMEGA[0] * e[:, 0, None])
        for d in range(1, 6):
            acc = acc + X[:, d, :] * -(OMEGA[d] * e[:, d, None])
        return acc

    Hxx, bx, Hab = [upper(prod(J[0], J[0])), upper(prod(J[1], J[1]))], [rhs(J[0]), rhs(J[1])], prod(J[0], J[1])
    Kf = int((free_of >= 0).sum())
    n = 4 * Kf
    H, b = np.zeros((n, n)), np.zeros(n)
    diag, rh, off = {}, {}, {}
    for a in range(E):
        i, j = free_of[v0[a]], free_of[v1[a]]
        if i >= 0:
            diag.setdefault(i, []).append(Hxx[0][a]); rh.setdefault(i, []).append(bx[0][a])
        if j >= 0:
            diag.setdefault(j, []).append(Hxx[1][a]); rh.setdefault(j, []).append(bx[1][a])
        if i >= 0 and j >= 0:
            if i < j:
                off.setdefault((i, j), []).append(Hab[a])
            else:
                off.setdefault((j, i), []).append(Hab[a].T)
    for i, terms in diag.items():
        H[4 * i:4 * i + 4, 4 * i:4 * i + 4] = ordered_sum(terms, order)
        b[4 * i:4 * i + 4] = ordered_sum(rh[i], order)
    for (i, j), terms in off.items():
        blk = ordered_sum(terms, order)
        H[4 * i:4 * i + 4, 4 * j:4 * j + 4] = blk
        H[4 * j:4 * j + 4, 4 * i:4 * i + 4] = blk.T
    return cost, H, b


def cost_at(sc, st, act, order, nudge):
    if not len(act):
        return 0.0
    v0, v1 = sc["v0"][act], sc["v1"][act]
    e = edge_errors(st["Rcw"][v0], st["tcw"][v0], st["Rcw"][v1], st["tcw"][v1], sc["meas"][act], nudge)
    return ordered_sum(chi2_of(e), order)


def optimize(sc, variant=VARIANTS[0], iterations=ITERATIONS, trace=None):
    """optimizer.optimize(20): sparse_optimizer.cpp:376-389 over levenberg.cpp:61-170 -> dict(poses [N, 12], status, iterations,
    trials, rejected_trials, solver_failures, stop, chi2_initial, chi2_final, lambda_final, lambda_initial, accepted, state)"""
    order, nudge, solver, ortho = variant
    st = initial_state(sc)
    act, free_of, vof = active_set(sc)
    tab = perturbation_table(nudge, ortho)
    r = dict(status=0, iterations=0, trials=0, rejected_trials=0, solver_failures=0, stop=0, chi2_initial=0.0, chi2_final=0.0,
             lambda_final=0.0, lambda_initial=0.0, accepted=0)
    lam, ni, n_bad, ok = 0.0, 2.0, 0, len(act) > 0
    it = 0
    while it < iterations and ok:
        current, H, b = linearise(sc, st, act, free_of, tab, order, nudge)
        if trace is not None:
            trace.append(dict(H=H, b=b, cost=current))
        ini = current
        if it == 0:
            r["chi2_initial"] = current
            lam = r["lambda_initial"] = TAU * float(np.abs(np.diag(H)).max())  # computeLambdaInit (:172-186): no user value here
            ni, n_bad = 2.0, 0
        rho, qmax = 0.0, 0
        x = np.zeros(len(b))
        while True:
            S = H + lam * np.eye(len(b))
            if solver == "lapack":
                xs, ok2 = np.linalg.solve(S, b), True
            else:
                xs, ok2 = ldlt_solve(S, b)
            if ok2:
                x = xs
            else:
                r["solver_failures"] += 1
            u = x.reshape(-1, 4)
            z = np.zeros(len(vof))
            trial = update_w(sc, st, vof, exp_so3(z, z, u[:, 0], nudge, ortho), u[:, 1:4])   # update (sparse_optimizer.cpp:422-441)
            temp = cost_at(sc, trial, act, order, nudge)
            if not ok2:
                temp = DBL_MAX
            rho = current - temp
            scale = 0.0
            for j in range(len(b)):
                scale += x[j] * (lam * x[j] + b[j])
            scale += 1e-3
            rho /= scale
            r["trials"] += 1
            if rho > 0 and math.isfinite(temp):
                y = 2 * rho - 1
                alpha = min(1. - (y * y) * y, 2. / 3.)
                lam *= max(1. / 3., alpha)
                ni = 2.0
                current = temp
                st = trial
                r["accepted"] += 1
            else:
                lam *= ni
                ni *= 2
                r["rejected_trials"] += 1
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        it += 1
        r["iterations"] = it
        r["chi2_final"] = current
        if qmax == 10 or rho == 0:
            ok, r["stop"] = False, 1
            continue
        n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
        if n_bad >= 3:
            ok, r["stop"] = False, 2
    if r["iterations"] == 0:
        r["chi2_final"] = r["chi2_initial"]
    r["lambda_final"] = lam
    out = np.concatenate([sc["Rcw"].reshape(-1, 9), sc["tcw"]], 1)   # a vertex outside the system repeats its input
    out[vof] = poses_of(st)[vof]
    r["poses"] = out
    r["state"] = st
    return r


COUNTS = ("status", "iterations", "trials", "rejected_trials", "solver_failures", "stop")


def counts(r):
    return tuple(int(r[k]) for k in COUNTS)


def pose_difference(a, b):
    """the largest difference of an entry of two pose arrays [N, 12]: a rotation entry's is absolute, a translation's is taken
    relative to the largest translation"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    if not len(a):
        return 0.0
    tscale = max(1.0, float(np.abs(b[:, 9:]).max()))
    return float(max(np.abs(a[:, :9] - b[:, :9]).max(), np.abs(a[:, 9:] - b[:, 9:]).max() / tscale))


def lambda_agrees(a, b):
    """lambda_initial is 1e-5 times a sum of squared Jacobian entries: it carries the Jacobian's noise, relative"""
    return abs(a - b) <= bound() * max(abs(a), abs(b))


# --------------------------------------------------------------------------------------------------------------- the scenes
def _rot(w):
    return exp_so3([w[0]], [w[1]], [w[2]])[0]


# camera in the body: the usual axis swap (camera z forward, x right) times a few degrees, and a lever arm
RCB = mm(_rot([0.03, -0.02, 0.015])[None], np.array([[[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]]))[0]
TCB = np.array([0.05, -0.02, 0.11])


def _f32(a):
    return np.asarray(a, np.float32).astype(F64)


def make_graph(seed, n, edges, fixed, noise=(2e-3, 1e-2), perturb=(5e-2, 1e-1), spacing=1.0, corrected=lambda k: k % 3 == 2,
               tcb=TCB, Rcb=RCB):
    """n planted body poses along a gently turning path (yaw, a little roll and pitch).  Measurements dRij, dtij from the planted
    camera poses, the rotation times Exp(noise), the translation plus noise.  The estimates are the planted body poses moved by
    a yaw about the world's z and a translation, which is all the optimisation can take back; a fixed vertex keeps the planted
    pose.  Vertex k is built like ImuCamPose(Rwc, twc, pKF) where corrected(k) (everything derived from Rwc, twc in double), and
    like ImuCamPose(pKF) elsewhere: Rwb, twb, Rcw, tcw each a float widened, so the camera pose is NOT the one the body pose
    implies, by a float rounding."""
    rng = np.random.default_rng(seed)
    fixed = np.array([1 if k in fixed else 0 for k in range(n)], np.int32)
    Rcb_f, tcb_f = _f32(Rcb), _f32(tcb)                                       # mImuCalib.mTcb is float
    sc = dict(Rcw=np.zeros((n, 3, 3)), tcw=np.zeros((n, 3)), Rwb=np.zeros((n, 3, 3)), twb=np.zeros((n, 3)),
              Rcb=np.tile(Rcb_f, (n, 1, 1)), tcb=np.tile(tcb_f, (n, 1)), fixed=fixed)
    true_R, true_t = np.zeros((n, 3, 3)), np.zeros((n, 3))
    for k in range(n):
        Rwb = mm(_rot([0.0, 0.0, 0.05 * k])[None], _rot([0.02 * math.sin(k), 0.015 * math.cos(0.7 * k), 0.0])[None])[0]
        twb = np.array([spacing * k * math.cos(0.02 * k), spacing * k * math.sin(0.02 * k), 0.1 * math.sin(0.3 * k)])
        Rbw = Rwb.T
        true_R[k], true_t[k] = Rcb_f @ Rbw, Rcb_f @ (-(Rbw @ twb)) + tcb_f     # the planted camera pose
        if not fixed[k]:
            Rwb = _rot([0.0, 0.0, rng.normal(0, 1) * perturb[0]]) @ Rwb
            twb = twb + rng.normal(0, 1, 3) * perturb[1]
        Rbw = Rwb.T
        Rcw, tcw = Rcb_f @ Rbw, Rcb_f @ (-(Rbw @ twb)) + tcb_f
        if corrected(k):                                                       # G2oTypes.cc:121-146 from Rwc, twc
            Rwc = Rcw.T.copy()
            twc = -(Rwc @ tcw)
            sc["twb"][k] = mv(Rwc, tcb_f) + twc
            sc["Rwb"][k] = mm(Rwc, Rcb_f)
            sc["Rcw"][k] = Rwc.T
            sc["tcw"][k] = -mv(sc["Rcw"][k], twc)
        else:                                                                  # G2oTypes.cc:25-71: four floats of the KeyFrame
            sc["Rwb"][k], sc["twb"][k], sc["Rcw"][k], sc["tcw"][k] = _f32(Rwb), _f32(twb), _f32(Rcw), _f32(tcw)
    sc["v0"] = np.array([e[0] for e in edges], np.int32)
    sc["v1"] = np.array([e[1] for e in edges], np.int32)
    meas = np.zeros((len(edges), 12))
    for e, (i, j) in enumerate(edges):
        dR = true_R[i] @ true_R[j].T
        dt = true_R[i] @ (-(true_R[j].T @ true_t[j])) + true_t[i]
        if any(noise):
            dR = _rot(rng.normal(0, 1, 3) * noise[0]) @ dR
            dt = dt + rng.normal(0, 1, 3) * noise[1]
        meas[e, :9], meas[e, 9:] = dR.reshape(9), dt
    sc["meas"] = meas
    sc["true"] = np.concatenate([true_R.reshape(n, 9), true_t], 1)
    return sc


def _chain(n, extra=()):
    return [(k + 1, k) for k in range(n - 1)] + list(extra)   # the mPrevKF arm: vertex 0 is the KeyFrame, vertex 1 its predecessor


def _loops(n, step, seed):
    rng = np.random.default_rng(seed)
    extra = [(k, k - int(rng.integers(2, 6))) for k in range(6, n, step)] + [(n - 1, 0)]
    return _chain(n, extra)


def _scene_hub():
    """vertex 1 has 70 neighbours in both directions, and 66 more edges to vertex 2 alone: an incident list of 137 and a pair
    list of 67, both longer than a wavefront"""
    edges = [(1, k) if k % 2 else (k, 1) for k in range(2, 72)] + [(1, 0)] + [(k + 1, k) for k in range(2, 71, 5)]
    edges += [(1, 2) if m % 2 else (2, 1) for m in range(66)]
    return make_graph(8, 72, edges, {0}, spacing=0.2)


def _scene_at_optimum():
    """exact measurements and the planted poses for a start, every vertex consistent: each rotation residual is the identity to
    a rounding, so LogSO3 leaves by an early exit (costheta above 1, or a sine below 1e-5) and no trial can gain"""
    return make_graph(37, 8, _chain(8, [(7, 0), (6, 2)]), {0}, noise=(0.0, 0.0), perturb=(0.0, 0.0), corrected=lambda k: True)


def _scene_radian():
    """two measurements of one pair that differ by a rotation of two radians about an axis the update cannot reach: the
    residuals stay near a radian each, LogSO3's general exit"""
    sc = make_graph(31, 6, _chain(6, [(2, 0), (2, 0), (5, 3), (5, 3)]), {0}, noise=(1e-3, 1e-2))
    for e, w in ((6, [1.0, 0.3, 0.2]), (8, [-0.4, 1.1, 0.3])):
        sc["meas"][e, :9] = (_rot(w) @ _rot(w) @ sc["meas"][e, :9].reshape(3, 3)).reshape(9)
    return sc


_BUILDERS = {
    "one_free": lambda: make_graph(1, 2, [(1, 0)], {0}),
    "three_edges": lambda: make_graph(2, 3, [(1, 0), (2, 1), (2, 0)], {0}),
    "one_sided": lambda: make_graph(10, 6, [(0, 1), (2, 0), (2, 1), (5, 3), (4, 5), (4, 3), (3, 2)], {0, 5}),
    "active_set": lambda: make_graph(9, 9, _chain(6, [(6, 7), (5, 0)]), {0, 6, 7}),          # (6, 7): both fixed; 8: no edge
    "duplicate_edges": lambda: make_graph(7, 6, _chain(6, [(3, 1), (3, 1), (1, 3), (5, 0), (3, 1)]), {0}),
    "hub70": _scene_hub,
    "kf11": lambda: make_graph(11, 12, _chain(12, [(11, 0), (8, 3)]), {0}),
    "kf12": lambda: make_graph(12, 13, _chain(13, [(12, 0), (9, 2)]), {0}),
    "kf13": lambda: make_graph(13, 14, _chain(14, [(13, 0), (7, 1)]), {0}),
    "free150_loops": lambda: make_graph(14, 151, _loops(151, 7, 11), {0}, spacing=0.5),
    # a start 2.5 radians and 30 units away: ten accepted updates, so `its` reaches 5, and DR's zeroing happens, twice
    "ten_updates": lambda: make_graph(17, 16, _chain(16, [(15, 0), (8, 2)]), {0}, noise=(2e-2, 1e-1), perturb=(2.5, 30.0)),
    "at_optimum": _scene_at_optimum,
    "noisy_nbad": lambda: make_graph(51, 8, _chain(8, [(7, 0), (5, 1)]), {0}, noise=(2e-2, 1e-1)),
    "radian": _scene_radian,
    "keyframe_built": lambda: make_graph(16, 7, _chain(7, [(6, 0), (5, 2)]), {0}, corrected=lambda k: False),
    "corrected_built": lambda: make_graph(17, 7, _chain(7, [(6, 0), (5, 2)]), {0}, corrected=lambda k: True),
}
GPU_SCENES = tuple(_BUILDERS)
# Once one of these small graphs has converged (three steps), a further trial moves the cost in its last digits only, and whether
# it is accepted is decided by rounding: the variants then disagree on the rejected trials.  They run optimize(3), every step of
# which is a large gain (as section 17's small scenes do); the others run the reference's optimize(20) to their own exit.
SHORT = {"one_free": 3, "three_edges": 3, "one_sided": 3}
_scene_cache, _ref_cache = {}, {}


def scene(name):
    if name not in _scene_cache:
        _scene_cache[name] = _BUILDERS[name]()
        _scene_cache[name]["iterations"] = SHORT.get(name, ITERATIONS)
    return _scene_cache[name]


def reference(name, variant=VARIANTS[0]):
    """the restatement's result for a scene, computed once"""
    key = (name, variant)
    if key not in _ref_cache:
        _ref_cache[key] = optimize(scene(name), variant, scene(name)["iterations"])
    return _ref_cache[key]


def digest(sc):
    h = hashlib.sha256()
    for k in ("Rcw", "tcw", "Rwb", "twb", "Rcb", "tcb", "fixed", "v0", "v1", "meas"):
        h.update(np.ascontiguousarray(sc[k]).tobytes())
    return h.hexdigest()[:16]


def vertex_records(sc):
    """the scene in the argument order of msorb.eg4_vertices"""
    return sc["Rcw"], sc["tcw"], sc["Rwb"], sc["twb"], sc["Rcb"], sc["tcb"], sc["fixed"]


def input_poses(sc):
    return np.concatenate([sc["Rcw"].reshape(-1, 9), sc["tcw"]], 1)


# --------------------------------------------------------------------- files of tests/essential_graph4_main.cc (native endianness)
def write_scenes(path, scenes):
    """n_scenes | per scene: N E iterations (int32) | vertices [N, 36] f64 (Rcw tcw Rwb twb Rcb tcb) | fixed [N] v0 [E] v1 [E] int32 |
    meas [E, 12] f64"""
    with open(path, "wb") as f:
        f.write(np.array([len(scenes)], np.int32).tobytes())
        for sc in scenes:
            n = len(sc["fixed"])
            f.write(np.array([n, len(sc["v0"]), sc.get("iterations", ITERATIONS)], np.int32).tobytes())
            rec = np.concatenate([sc[k].reshape(n, -1) for k in ("Rcw", "tcw", "Rwb", "twb", "Rcb", "tcb")], 1)
            f.write(np.ascontiguousarray(rec, F64).tobytes())
            for k in ("fixed", "v0", "v1"):
                f.write(np.ascontiguousarray(sc[k], np.int32).tobytes())
            f.write(np.ascontiguousarray(sc["meas"], F64).tobytes())


def read_results(path, scenes):
    """per scene: 6 int32 (COUNTS) | chi2_initial chi2_final lambda_final lambda_initial f64 | poses [N, 12] f64"""
    out = []
    with open(path, "rb") as f:
        for sc in scenes:
            c = np.frombuffer(f.read(24), np.int32)
            d = np.frombuffer(f.read(32), F64)
            n = len(sc["fixed"])
            poses = np.frombuffer(f.read(96 * n), F64).reshape(n, 12)
            r = dict(zip(COUNTS, (int(v) for v in c)))
            r.update(chi2_initial=float(d[0]), chi2_final=float(d[1]), lambda_final=float(d[2]), lambda_initial=float(d[3]), poses=poses)
            out.append(r)
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def bound():
    """what the device and the host program may differ by from the forward restatement"""
    return MARGIN * golden()["D"]


def scene_bound(name):
    """the same margin over the scene's OWN recorded spread: D is set by the largest scene, and on a small one 16 D would let a wrong
    pose through.  The floor is one rounding of an entry of size one: a scene on which every variant returns the same bits still
    allows the last bit"""
    return MARGIN * max(golden()["scenes"][name]["spread"], float(np.finfo(F64).eps))


def measure():
    g = dict(scenes={}, D=0.0)
    for name in GPU_SCENES:
        rs = [reference(name, v) for v in VARIANTS]
        cs = {counts(r) for r in rs}
        dd = max(pose_difference(a["poses"], b["poses"]) for a in rs for b in rs)
        lams = [r["lambda_initial"] for r in rs]
        g["scenes"][name] = dict(digest=digest(scene(name)), iterations=scene(name)["iterations"], counts=list(counts(rs[0])),
                                 variants_agree=len(cs) == 1, spread=dd, accepted=rs[0]["accepted"], chi2_initial=rs[0]["chi2_initial"],
                                 chi2_final=rs[0]["chi2_final"], lambda_initial=rs[0]["lambda_initial"],
                                 lambda_initial_spread=(max(lams) - min(lams)) / max(max(lams), DBL_MAX ** -1))
        g["D"] = max(g["D"], dd)
        print(name, counts(rs[0]), "agree" if len(cs) == 1 else f"DISAGREE {sorted(cs)}", f"accepted {rs[0]['accepted']} spread {dd:.3e}",
              f"chi2 {rs[0]['chi2_initial']:.3e} -> {rs[0]['chi2_final']:.3e} lambda0 {rs[0]['lambda_initial']:.3e}", flush=True)
    return g


if __name__ == "__main__":
    g = measure()
    if "--measure" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(g, f, indent=1)
            f.write("\n")
    print("D =", g["D"])
