"""Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:4422-4779) and PoseInertialOptimizationLastFrame (:4781-5172)
after their gathering loops, restated in float64 / float32 numpy for pinhole mono / stereo frames without a second camera:
EdgeMonoOnlyPose / EdgeStereoOnlyPose (include/G2oTypes.h:390-493, src/G2oTypes.cc:375-490), EdgeInertial (G2oTypes.cc:492-594),
EdgeGyroRW / EdgeAccRW (G2oTypes.h:635-704), EdgePriorPoseImu (G2oTypes.cc:720-760), ImuCamPose (G2oTypes.cc:73-119, :192-220),
Gauss-Newton (optimization_algorithm_gauss_newton.cpp:50-93 under sparse_optimizer.cpp:354-419), a BaseMultiEdge's quadratic form
(base_multi_edge.hpp:171-222), Marginalize (Optimizer.cc:2975-3048) and ConstraintPoseImu's constructor (G2oTypes.h:711-722); the
scene generator and the scene list of the GPU tests.  No GPU, no library and no code shared with
ms-slam_amd/csrc/pose_inertial_device.h: the visual edges are evaluated in one array pass, the multi-edges as whole matrices.  The
SO3 functions, the float32 preintegration and the ordered sums are those of tests/inertial_opt_cases.py.

What the restatement fixes where the reference leaves it to Eigen / libm, and the variants that measure what that moves
(`python tests/pose_inertial_cases.py --measure` writes tests/golden/pose_inertial_sensitivity.json):
  * `sum_order`: how the visual edges' terms, the products of the quadratic forms and the edges' contributions to H and b are
    added: 'forward', 'reverse', 'pairwise' (numpy's matmul and sum);
  * `solver`: 'ldlt' (unpivoted square-root-free L D L^T, a pivot !(d > 0) fails) or 'lapack' (numpy.linalg.cholesky / solve);
  * `nudge`: sin, cos, acos and their float32 forms one ulp up: what another libm may return;
  * `ortho`: NormalizeRotation (float32 and float64) as U V^T of numpy's SVD, or by Newton's polar iteration;
  * `post`: Marginalize's pseudo-inverse and the constructor's eigen-decomposition through numpy.linalg.svd + eigh, or a cyclic Jacobi.
The first of VARIANTS is THE restatement.
"""
import functools
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from inertial_opt_cases import (F32, F64, GRAVITY, I3, EDGE_DTYPE, _rot, _up, exp_so3, hat, info_from_covariance, integrate,  # noqa: E402
                                inverse_right_jacobian, jacobi_eigh, log_so3, mm, mv, normalize_rotation, ordered_matmul,
                                ordered_sum, right_jacobian, so3f_exp, tr)

MARGIN = 16                        # the project's margin over the measured spread (DESIGN.md sections 9 to 19)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_inertial_sensitivity.json")
VARIANTS = (("forward", "ldlt", False, "svd", "lapack"), ("reverse", "ldlt", False, "svd", "lapack"),
            ("pairwise", "ldlt", False, "svd", "lapack"), ("forward", "lapack", False, "svd", "lapack"),
            ("forward", "ldlt", True, "svd", "lapack"), ("forward", "ldlt", False, "polar", "lapack"),
            ("forward", "ldlt", False, "svd", "jacobi"))
#            (sum_order, solver, nudge, ortho, post)
QUANTITIES = ("Rwb", "twb", "v", "bg", "ba", "chi2", "H_raw", "H_prior")

STATE_DTYPE = np.dtype([("Rwb", "<f8", 9), ("twb", "<f8", 3), ("v", "<f8", 3), ("bg", "<f8", 3), ("ba", "<f8", 3)])
PROBLEM_DTYPE = np.dtype([("form", "<i4"), ("rec_init", "<i4"), ("n", "<i4"), ("reserved", "<i4"), ("frame", STATE_DTYPE),
                          ("other", STATE_DTYPE), ("prior", STATE_DTYPE), ("Rcw", "<f8", 9), ("tcw", "<f8", 3), ("Rcb", "<f8", 9),
                          ("tcb", "<f8", 3), ("tbc", "<f8", 3), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                          ("mbf", "<f4"), ("reserved_f", "<f4"), ("pre", EDGE_DTYPE), ("info_gyro", "<f8", 9),
                          ("info_acc", "<f8", 9), ("H", "<f8", 225)])
RESULT_DTYPE = np.dtype([("est", STATE_DTYPE), ("Rwb_f", "<f4", 9), ("twb_f", "<f4", 3), ("v_f", "<f4", 3), ("n_initial", "<i4"),
                         ("n_bad", "<i4"), ("n_inliers", "<i4"), ("iterations", "<i4", 4), ("solve_failed", "<i4", 4),
                         ("H_raw", "<f8", 900), ("H_prior", "<f8", 225)])
assert (STATE_DTYPE.itemsize, PROBLEM_DTYPE.itemsize, RESULT_DTYPE.itemsize) == (168, 3632, 9272)

KITTI = dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, mbf=386.1448)
CHI2_MONO = ((12.0, 7.5, 5.991, 5.991), (5.991, 5.991, 5.991, 5.991))          # Optimizer.cc:4623, :4999, as floats below
CHI2_STEREO = (15.6, 9.8, 7.815, 7.815)                                        # :4624, :5000


# ------------------------------------------------------------------------------------------------ the vertices
def _camera(st, Rcb, tcb):
    """ImuCamPose::Update's camera pose (G2oTypes.cc:211-218)"""
    Rbw = st["Rwb"].T.copy()
    tbw = mv(-Rbw, st["twb"])
    st["Rcw"] = mm(Rcb, Rbw)
    st["tcw"] = mv(Rcb, tbw) + tcb


def _vertices(s):
    return dict(Rwb=s["Rwb"].reshape(3, 3).astype(F64), twb=s["twb"].astype(F64), v=s["v"].astype(F64), bg=s["bg"].astype(F64),
                ba=s["ba"].astype(F64), its=0)


def _update(st, u, Rcb, tcb, nudge, ortho):
    """VertexPose / VertexVelocity / VertexGyroBias / VertexAccBias oplusImpl; ImuCamPose::Update (G2oTypes.cc:192-220)"""
    st["twb"] = st["twb"] + mv(st["Rwb"], u[3:6])                              # :199, the old Rwb
    R = mm(st["Rwb"], exp_so3(u[0], u[1], u[2], nudge, ortho))                 # :200
    st["its"] += 1
    if st["its"] >= 3:                                                         # :203-208
        R = normalize_rotation(R, ortho)
        st["its"] = 0
    st["Rwb"] = R
    _camera(st, Rcb, tcb)
    st["v"] = st["v"] + u[6:9]
    st["bg"] = st["bg"] + u[9:12]
    st["ba"] = st["ba"] + u[12:15]


# ------------------------------------------------------------------------------------------------ the visual edges
def visual_errors(sc, F):
    """computeError of both edges (G2oTypes.h:401-405, :477-481; G2oTypes.cc:170-185; Pinhole.cpp:35-41) -> e [n, 3], Xc, chi2"""
    p = sc["problem"]
    fx, fy, cx, cy, bf = (float(p[k]) for k in ("fx", "fy", "cx", "cy", "mbf"))
    Xw = sc["pos"].astype(F64)
    Xc = mv(F["Rcw"][None], Xw) + F["tcw"][None]
    w = sc["inv"].astype(F64)
    stereo = sc["ur"] >= 0
    p0 = (fx * Xc[:, 0]) / Xc[:, 2] + cx
    p1 = (fy * Xc[:, 1]) / Xc[:, 2] + cy
    e = np.zeros((len(Xw), 3))
    e[:, 0] = sc["xy"][:, 0].astype(F64) - p0
    e[:, 1] = sc["xy"][:, 1].astype(F64) - p1
    e[:, 2] = np.where(stereo, sc["ur"].astype(F64) - (p0 - bf * (1 / Xc[:, 2])), 0.0)
    c2 = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
    chi2 = np.where(stereo, c2 + e[:, 2] * (w * e[:, 2]), c2)
    return e, Xc, chi2


def visual_jacobians(sc, Xc):
    """linearizeOplus (G2oTypes.cc:375-395, :429-454): (proj_jac Rcb) SE3deriv(Xb) -> J [n, 3, 6] (row 2 zero for a mono edge)"""
    p = sc["problem"]
    fx, fy, bf = float(p["fx"]), float(p["fy"]), float(p["mbf"])
    Rcb, tbc = p["Rcb"].reshape(3, 3), p["tbc"]
    n = len(Xc)
    stereo = sc["ur"] >= 0
    Xb = mv(Rcb.T[None], Xc) + tbc[None]
    zz = Xc[:, 2] * Xc[:, 2]
    pj = np.zeros((n, 3, 3))
    pj[:, 0, 0] = fx / Xc[:, 2]
    pj[:, 0, 2] = (-fx * Xc[:, 0]) / zz
    pj[:, 1, 1] = fy / Xc[:, 2]
    pj[:, 1, 2] = (-fy * Xc[:, 1]) / zz
    pj[:, 2, 0] = np.where(stereo, pj[:, 0, 0], 0.0)
    pj[:, 2, 2] = np.where(stereo, pj[:, 0, 2] + bf * (1.0 / zz), 0.0)
    M = mm(pj, Rcb[None])
    D = np.zeros((n, 3, 6))
    x, y, z = Xb[:, 0], Xb[:, 1], Xb[:, 2]
    D[:, 0, 1], D[:, 0, 2], D[:, 1, 0], D[:, 1, 2], D[:, 2, 0], D[:, 2, 1] = z, -y, -z, x, y, -x
    D[:, 0, 3] = D[:, 1, 4] = D[:, 2, 5] = 1.0
    return (M[:, :, 0, None] * D[:, None, 0, :] + M[:, :, 1, None] * D[:, None, 1, :]) + M[:, :, 2, None] * D[:, None, 2, :]


def huber(chi2, delta, robust):
    """RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91) -> rho[1]"""
    if not robust:
        return np.ones_like(chi2)
    dsqr = delta * delta
    lin = chi2 > dsqr
    return np.where(lin, delta / np.sqrt(np.where(lin, chi2, 1.0)), 1.0)


def visual_forms(sc, J, e, rho1, mask, order, with_b=True):
    """sum over the masked edges of A^T (rho1 Omega) A [6, 6] and -(A^T (rho1 Omega) e) [6]"""
    w = sc["inv"].astype(F64)
    wr = (rho1 * w)[:, None, None]
    stereo = (sc["ur"] >= 0)[:, None, None]
    H2 = (J[:, 0, :, None] * wr) * J[:, 0, None, :] + (J[:, 1, :, None] * wr) * J[:, 1, None, :]
    H = np.where(stereo, H2 + (J[:, 2, :, None] * wr) * J[:, 2, None, :], H2)
    Hs = ordered_sum(H[mask], order)
    if not with_b:
        return Hs, None
    r1, w1 = rho1[:, None], w[:, None]
    b2 = ((r1 * J[:, 0, :]) * w1) * e[:, 0, None] + ((r1 * J[:, 1, :]) * w1) * e[:, 1, None]
    b = np.where(stereo[:, :, 0], b2 + ((r1 * J[:, 2, :]) * w1) * e[:, 2, None], b2)
    return Hs, -ordered_sum(b[mask], order)


# ------------------------------------------------------------------------------------------------ the multi-edges
def inertial_edge(sc, F, O, nudge, ortho, jac=True):
    """EdgeInertial::computeError (G2oTypes.cc:514-534) and linearizeOplus (:536-594): 1 = the other end, 2 = the frame.
    -> e [9], J [9, 24] in GetHessian's column order (P1 6, V1 3, G1 3, A1 3, P2 6, V2 3)"""
    pre = sc["problem"]["pre"]
    m = {k: pre[k].reshape(3, 3) for k in ("dR", "JRg", "JVg", "JVa", "JPg", "JPa")}
    dbg = F32(O["bg"]) - pre["bias"][3:6]                                      # GetDeltaBias (ImuTypes.cc:277-308), float
    dba = F32(O["ba"]) - pre["bias"][0:3]
    assert dbg.dtype == F32 and dba.dtype == F32
    dR = normalize_rotation(mm(m["dR"], so3f_exp(mv(m["JRg"], dbg)[None], nudge)[0]), ortho).astype(F64)
    dV = ((pre["dV"] + mv(m["JVg"], dbg)) + mv(m["JVa"], dba)).astype(F64)
    dP = ((pre["dP"] + mv(m["JPg"], dbg)) + mv(m["JPa"], dba)).astype(F64)
    g = np.array([0.0, 0.0, -GRAVITY])
    dt = float(pre["dT"])
    Rbw1 = O["Rwb"].T.copy()
    eR = mm(mm(dR.T.copy(), Rbw1), F["Rwb"])                                   # :528
    er = log_so3(eR[None], nudge)[0]
    tv = (F["v"] - O["v"]) - g * dt
    tp = ((F["twb"] - O["twb"]) - O["v"] * dt) - ((g * dt) * dt) / 2
    e = np.concatenate([er, mv(Rbw1, tv) - dV, mv(Rbw1, tp) - dP])
    if not jac:
        return e, None
    J = np.zeros((9, 24))
    invJr = inverse_right_jacobian(er[None], nudge)[0]
    J[0:3, 0:3] = mm(mm(-invJr, F["Rwb"].T.copy()), O["Rwb"])                  # :561
    J[3:6, 0:3] = hat(mv(Rbw1, tv))                                            # :562
    J[6:9, 0:3] = hat(mv(Rbw1, ((F["twb"] - O["twb"]) - O["v"] * dt) - ((0.5 * g) * dt) * dt))   # :563-564
    J[6:9, 3:6] = -I3                                                          # :566
    J[3:6, 6:9] = -Rbw1                                                        # :570
    J[6:9, 6:9] = -Rbw1 * dt                                                   # :571
    JRg = m["JRg"].astype(F64)
    RJ = right_jacobian(mv(JRg, dbg.astype(F64))[None], nudge)[0]
    J[0:3, 9:12] = mm(mm(mm(-invJr, eR.T.copy()), RJ), JRg)                    # :575
    J[3:6, 9:12] = -m["JVg"].astype(F64)
    J[6:9, 9:12] = -m["JPg"].astype(F64)
    J[3:6, 12:15] = -m["JVa"].astype(F64)
    J[6:9, 12:15] = -m["JPa"].astype(F64)
    J[0:3, 15:18] = invJr                                                      # :587
    J[6:9, 18:21] = mm(Rbw1, F["Rwb"])                                         # :589
    J[3:6, 21:24] = Rbw1                                                       # :593
    return e, J


def prior_edge(sc, O, nudge, jac=True):
    """EdgePriorPoseImu::computeError (G2oTypes.cc:731-745) and linearizeOplus (:747-760) -> e [15], J [15, 15]"""
    pr = sc["problem"]["prior"]
    Rt = pr["Rwb"].reshape(3, 3).T.copy()
    A = mm(Rt, O["Rwb"])
    er = log_so3(A[None], nudge)[0]
    e = np.concatenate([er, mv(Rt, O["twb"] - pr["twb"]), O["v"] - pr["v"], O["bg"] - pr["bg"], O["ba"] - pr["ba"]])
    if not jac:
        return e, None
    J = np.eye(15)
    J[0:3, 0:3] = inverse_right_jacobian(er[None], nudge)[0]
    J[3:6, 3:6] = A
    return e, J


def quadratic(J, info, e, order):
    """computeQuadraticForm (base_multi_edge.hpp:171-222): (A^T omega) B for every pair, A^T (-(omega e))"""
    AtO = ordered_matmul(J.T[None], info[None], order)[0]
    H = ordered_matmul(AtO[None], J[None], order)[0]
    if e is None:
        return H, None
    Oe = ordered_matmul(info[None], e[None, :, None], order)[0, :, 0]
    return H, ordered_matmul(J.T[None], -Oe[None, :, None], order)[0, :, 0]


def _add(parts, order):
    return ordered_sum(np.stack(parts), order)


# unknowns: the frame's fifteen, then the other end's; EdgeInertial's columns -> unknowns
def _inertial_map(form):
    idx = np.full(24, -1)
    idx[15:24] = np.arange(9)
    if form == 1:
        idx[0:15] = 15 + np.arange(15)
    return idx


def ldlt_solve(A, b):
    """unpivoted square-root-free L D L^T; None: a pivot that is not > 0"""
    n = len(A)
    A = A.copy()
    y = b.copy()
    L = np.eye(n)
    d = np.zeros(n)
    for j in range(n):
        d[j] = A[j, j]
        if not d[j] > 0:
            return None
        L[j + 1:, j] = A[j, j + 1:] * (1.0 / d[j])
        A[j + 1:, j + 1:] -= L[j + 1:, j, None] * A[j, None, j + 1:]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        s = y[i] * (1.0 / d[i])
        for m in range(i + 1, n):
            s -= L[m, i] * x[m]
        x[i] = s
    return x


def solve(H, b, solver):
    if solver == "ldlt":
        return ldlt_solve(H, b)
    Hs = np.triu(H) + np.triu(H, 1).T
    try:
        np.linalg.cholesky(Hs)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(Hs, b)


# ------------------------------------------------------------------------------------------------ Marginalize, ConstraintPoseImu
def marginalize(H, post):
    """Marginalize(H, 0, 14) (Optimizer.cc:2975-3048), the trailing 15x15 -> (Hc - Hcb pinv(Hb) Hbc, the 15 singular values)"""
    Hb = H[:15, :15]
    if post == "lapack":
        U, s, Vt = np.linalg.svd(Hb)
        inv = (Vt.T * np.where(s > 1e-6, 1.0 / np.where(s > 1e-6, s, 1.0), 0.0)[None, :]) @ U.T        # :3012-3018
    else:
        s, V = jacobi_eigh((Hb + Hb.T) / 2)
        keep = np.abs(s) > 1e-6
        inv = (V * np.where(keep, 1.0 / np.where(keep, s, 1.0), 0.0)[None, :]) @ V.T
        s = np.abs(s)
    return H[15:, 15:] - H[15:, :15] @ inv @ H[:15, 15:], np.sort(s)


def constraint_information(H, post):
    """ConstraintPoseImu's constructor (G2oTypes.h:711-722): SelfAdjointEigenSolver reads the lower triangle -> (H, eigenvalues)"""
    Hs = np.tril(H) + np.tril(H, -1).T
    w, V = np.linalg.eigh(Hs) if post == "lapack" else jacobi_eigh(Hs)
    return (V * np.where(w < 1e-12, 0.0, w)[None, :]) @ V.T, np.sort(w)


# ------------------------------------------------------------------------------------------------ the routine
def optimize(sc, variant=VARIANTS[0], stale=True):
    """One call.  stale=False: what the routine would return if an inlier's chi2 were taken at the returned estimate (the GPU
    scene `stale_chi2` must come out differently).
    -> dict(est, flags, n_bad, n_inliers, iterations, solve_failed, H_raw, H_prior, chi2 (every compared chi2 with its threshold),
    sigma, eigs, levels (the flags after every classification), prior_chi2 (the prior edge's chi2 of every pass), chi2_final
    (every edge's chi2 as the routine leaves it, with the threshold it was last compared with))"""
    order, solver, nudge, ortho, post = variant
    p = sc["problem"]
    form, n = int(p["form"]), int(p["n"])
    N = 30 if form == 1 else 15
    Rcb, tcb = p["Rcb"].reshape(3, 3), p["tcb"]
    F, O = _vertices(p["frame"]), _vertices(p["other"])
    F["Rcw"], F["tcw"] = p["Rcw"].reshape(3, 3).astype(F64), p["tcw"].astype(F64)   # G2oTypes.cc:95-96
    _camera(O, Rcb, tcb)
    info9, Ig, Ia, Hp = p["pre"]["info"].reshape(9, 9), p["info_gyro"].reshape(3, 3), p["info_acc"].reshape(3, 3), p["H"].reshape(15, 15)
    imap = _inertial_map(form)
    stereo = sc["ur"] >= 0
    close = sc["close"].astype(bool)
    d_mono, d_stereo = float(F32(math.sqrt(5.991))), float(F32(math.sqrt(7.815)))
    delta = np.where(stereo, d_stereo, d_mono)
    level = np.zeros(n, bool)
    chi2 = np.zeros(n)
    x = np.zeros(N)
    iterations, failed = [-1] * 4, [0] * 4
    compared, levels, prior_chi2 = [], [], []
    n_bad = n_inliers = 0

    def multi(F, O, robust_prior, with_b):
        """the multi-edges' H [N, N] parts and b parts, in the order inertial, gyro, acc, prior"""
        Hs, bs = [], []
        e, J = inertial_edge(sc, F, O, nudge, ortho)
        Hi, bi = quadratic(J, info9, e if with_b else None, order)
        sel = imap >= 0
        H = np.zeros((N, N))
        H[np.ix_(imap[sel], imap[sel])] = Hi[np.ix_(sel, sel)]
        Hs.append(H)
        if with_b:
            b = np.zeros(N)
            b[imap[sel]] = bi[sel]
            bs.append(b)
        for (info, lo, err) in ((Ig, 9, F["bg"] - O["bg"]), (Ia, 12, F["ba"] - O["ba"])):
            H, b = np.zeros((N, N)), np.zeros(N)
            H[lo:lo + 3, lo:lo + 3] = info
            Oe = mv(info, err)
            b[lo:lo + 3] = -Oe
            if form == 1:
                H[15 + lo:18 + lo, 15 + lo:18 + lo] = info
                H[lo:lo + 3, 15 + lo:18 + lo] = -info
                H[15 + lo:18 + lo, lo:lo + 3] = -info
                b[15 + lo:18 + lo] = Oe
            Hs.append(H)
            bs.append(b)
        if form == 1:
            e, J = prior_edge(sc, O, nudge)
            r1 = 1.0
            if robust_prior:
                Oe = ordered_matmul(Hp[None], e[None, :, None], order)[0, :, 0]
                c = float(ordered_sum(e * Oe, order))
                r1 = float(huber(np.array([c]), 5.0, True)[0])                  # Optimizer.cc:4992-4994
                prior_chi2.append(c)
            Hq, bq = quadratic(J, r1 * Hp, e if with_b else None, order)
            H, b = np.zeros((N, N)), np.zeros(N)
            H[15:, 15:] = Hq
            Hs.append(H)
            if with_b:
                b[15:] = bq
                bs.append(b)
        return Hs, bs

    for it in range(4):
        robust = it < 3                                                        # :4669-4670
        passes, ok = 0, True
        for _ in range(10):                                                    # gauss_newton.cpp:50-93
            e, Xc, c2 = visual_errors(sc, F)
            act = ~level
            chi2 = np.where(act, c2, chi2)                                     # computeActiveErrors
            J = visual_jacobians(sc, Xc)
            Hv, bv = visual_forms(sc, J, e, huber(c2, delta, robust), act, order)
            Hs, bs = multi(F, O, True, True)
            H0, b0 = np.zeros((N, N)), np.zeros(N)
            H0[:6, :6], b0[:6] = Hv, bv
            H = _add([H0] + Hs, order)
            b = _add([b0] + bs, order)
            sol = solve(H, b, solver)
            if sol is None:
                ok = False
                failed[it] = 1
            else:
                x = sol
            _update(F, x[:15], Rcb, tcb, nudge, ortho)                         # :85: also when the solve failed
            if form == 1:
                _update(O, x[15:], Rcb, tcb, nudge, ortho)
            passes += 1
            if not ok:
                break
        iterations[it] = passes
        e, Xc, c2 = visual_errors(sc, F)                                       # the classification (:4638-4700)
        chi2 = np.where(level, c2, chi2) if stale else c2
        cf = chi2.astype(F32)
        tm = F32(CHI2_MONO[form][it])
        tc = F32(1.5 * float(tm))
        thr = np.where(stereo, F32(CHI2_STEREO[it]), np.where(close, tc, tm)).astype(F32)
        depth_ok = (mv(F["Rcw"][None, 2:3], sc["pos"].astype(F64))[:, 0] + F["tcw"][2]) > 0.0
        level = (cf > thr) | (~stereo & ~depth_ok)
        compared.append((cf.astype(F64), thr.astype(F64)))
        levels.append(level.copy())
        n_bad = int(level.sum())
        n_inliers = n - n_bad
        if n + (4 if form == 1 else 3) < 10:                                   # :4702
            break
    flags = level.copy()
    last_thr = compared[-1][1]
    if n_inliers < 30 and not int(p["rec_init"]):                              # :4709-4733
        e, Xc, chi2 = visual_errors(sc, F)
        thr = np.where(stereo, 24.0, 18.0)
        below = chi2 < thr
        flags = flags & ~below
        n_bad = int((~below).sum())
        compared.append((chi2.copy(), thr))
        last_thr = thr
    e, Xc, c2 = visual_errors(sc, F)                                           # the Hessian (:4743-4773 / :5120-5162)
    J = visual_jacobians(sc, Xc)
    Hv, _ = visual_forms(sc, J, e, np.ones(n), ~flags, order, with_b=False)
    Hs, _ = multi(F, O, False, False)
    H0 = np.zeros((N, N))
    H0[:6, :6] = Hv
    H = _add(Hs + [H0], order)
    if form == 1:
        perm = np.concatenate([np.arange(15, 30), np.arange(15)])              # the previous frame first
        H_raw = H[np.ix_(perm, perm)]
        M, sigma = marginalize(H_raw, post)
    else:
        H_raw, M, sigma = H, H, np.zeros(15)
    H_prior, eigs = constraint_information(M, post)
    return dict(est=dict(Rwb=F["Rwb"], twb=F["twb"], v=F["v"], bg=F["bg"], ba=F["ba"]), flags=flags, n_bad=n_bad, n_inliers=n_inliers,
                iterations=iterations, solve_failed=failed, H_raw=H_raw, H_prior=H_prior, chi2=compared, sigma=sigma, eigs=eigs,
                levels=levels, prior_chi2=prior_chi2, chi2_final=(chi2.copy(), np.asarray(last_thr, F64)))


# ------------------------------------------------------------------------------------------------ scenes
def _state_record(rec, Rwb, twb, v, bg, ba):
    rec["Rwb"], rec["twb"], rec["v"], rec["bg"], rec["ba"] = np.asarray(Rwb).reshape(9), twb, v, bg, ba


def _f32(a):
    return np.asarray(a, F64).astype(F32).astype(F64)


RCB = _rot(np.array([0.01, -0.02, 0.015])) @ np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])   # body x forward -> camera z
TCB = np.array([0.05, -0.02, 0.1])


def make_step(rng, prev, n, form, mono_frac=0.3, outliers=0.0, noise_px=0.6, start=1.0, imu_noise=1.0, close_frac=None, behind=0,
              rec_init=0, prior=None, sub=6, dt=0.1 / 6, depth=(4.0, 40.0), bad_info=False, imu_sigma=1.0, outlier_bias=False):
    """One tracking frame after `prev` (a dict(Rwb, twb, v, bg, ba) of the true state): IMU samples integrated in float32, the frame's
    true state from that preintegration (so the inertial edge is consistent with the states up to the noise), n observations
    of points in front of the camera.  form 1 takes `prior` = dict(state=..., H=...), the result of the call before."""
    sig_g, sig_a = 1e-3 * imu_sigma, 1e-2 * imu_sigma
    g_w = np.array([0.0, 0.0, -GRAVITY])
    a_b = rng.normal(0, 0.8, 3)[None, :] + rng.normal(0, 0.2, (sub, 3))
    w_b = rng.normal(0, 0.15, 3)[None, :] + rng.normal(0, 0.03, (sub, 3))
    R, pos, vel = prev["Rwb"].copy(), prev["twb"].copy(), prev["v"].copy()
    acc, gyr = np.zeros((sub, 3)), np.zeros((sub, 3))
    for i in range(sub):
        acc[i] = a_b[i] + prev["ba"]
        gyr[i] = w_b[i] + prev["bg"]
        a_w = R @ a_b[i] + g_w
        pos = pos + vel * dt + 0.5 * a_w * dt * dt
        vel = vel + a_w * dt
        R = R @ _rot(w_b[i] * dt)
    bias = np.concatenate([prev["ba"], prev["bg"]]).astype(F32)
    pre = integrate((acc + imu_noise * sig_a * rng.normal(0, 1, (sub, 3))).astype(F32)[None],
                    (gyr + imu_noise * sig_g * rng.normal(0, 1, (sub, 3))).astype(F32)[None], dt, bias[0:3], bias[3:6],
                    [sig_g ** 2] * 3 + [sig_a ** 2] * 3)
    true = dict(Rwb=R, twb=pos, v=vel, bg=prev["bg"] + rng.normal(0, 1e-5, 3), ba=prev["ba"] + rng.normal(0, 1e-4, 3))
    p = np.zeros((), PROBLEM_DTYPE)
    p["form"], p["rec_init"], p["n"] = form, rec_init, n
    for k, v in KITTI.items():
        p[k] = v
    p["Rcb"], p["tcb"] = RCB.reshape(9), TCB
    p["tbc"] = _f32(-RCB.T @ TCB)                                              # mTbc.translation(), a float member of its own
    for f in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa"):
        p["pre"][f] = pre[f][0].reshape(-1)
    p["pre"]["dT"], p["pre"]["bias"] = pre["dT"], bias
    p["pre"]["info"] = info_from_covariance(pre["C"][0]).reshape(-1)
    T = float(pre["dT"])
    wg, wa = rng.normal(0, 0.1, (3, 3)), rng.normal(0, 0.1, (3, 3))
    Cg = (np.eye(3) + wg @ wg.T) * (1e-4 ** 2 * T)                             # the random-walk blocks of C, full 3x3
    Ca = (np.eye(3) + wa @ wa.T) * (1e-3 ** 2 * T)
    p["info_gyro"], p["info_acc"] = np.linalg.inv(_f32(Cg)).reshape(-1), np.linalg.inv(_f32(Ca)).reshape(-1)
    if bad_info:                                                               # an indefinite information: a pivot comes out negative
        p["pre"]["info"] = (-np.eye(9) * 1e6).reshape(-1)
    # the estimates the call starts from: floats widened (GetImuRotation() etc.)
    dRs = _rot(start * rng.normal(0, 0.004, 3))
    Rwb0 = _f32(true["Rwb"] @ dRs)
    twb0 = _f32(true["twb"] + start * rng.normal(0, 0.01, 3))
    _state_record(p["frame"], Rwb0, twb0, _f32(true["v"] + start * rng.normal(0, 0.02, 3)), _f32(prev["bg"]), _f32(prev["ba"]))
    Rcw0 = RCB @ Rwb0.T
    p["Rcw"], p["tcw"] = _f32(Rcw0).reshape(9), _f32(RCB @ (-Rwb0.T @ twb0) + TCB)   # GetPose() widened
    if form == 0:
        _state_record(p["other"], _f32(prev["Rwb"]), _f32(prev["twb"]), _f32(prev["v"]), _f32(prev["bg"]), _f32(prev["ba"]))
    else:
        s = prior["state"]
        _state_record(p["other"], _f32(s["Rwb"]), _f32(s["twb"]), _f32(s["v"]), _f32(s["bg"]), _f32(s["ba"]))
        s = prior.get("lin", s)
        _state_record(p["prior"], s["Rwb"], s["twb"], s["v"], s["bg"], s["ba"])
        p["H"] = np.asarray(prior["H"]).reshape(-1)
    # observations: points in the true camera frame
    Rcw_t = RCB @ true["Rwb"].T
    tcw_t = RCB @ (-true["Rwb"].T @ true["twb"]) + TCB
    z = rng.uniform(depth[0], depth[1], n)
    if close_frac is not None:
        k = int(round(close_frac * n))
        z[:k] = rng.uniform(3.0, 9.0, k)
        z[k:] = rng.uniform(12.0, 40.0, n - k)
    u, v = rng.uniform(30, 1200, n), rng.uniform(20, 350, n)
    Xc = np.stack([(u - KITTI["cx"]) / KITTI["fx"] * z, (v - KITTI["cy"]) / KITTI["fy"] * z, z], 1)
    if behind:
        Xc[-behind:, 2] = -rng.uniform(5.0, 20.0, behind)
    Xw = (Xc - tcw_t[None]) @ Rcw_t                                            # Rcw^T (Xc - tcw)
    lvl = rng.integers(0, 8, n)
    sigma = 1.2 ** lvl
    px = np.stack([u, v], 1) + noise_px * sigma[:, None] * rng.normal(0, 1, (n, 2))
    ur = u - KITTI["mbf"] / np.where(Xc[:, 2] > 0, Xc[:, 2], 10.0) + noise_px * sigma * rng.normal(0, 1, n)
    mono = rng.uniform(0, 1, n) < mono_frac
    if behind:
        mono[-behind:] = True
    nout = int(round(outliers * n))
    if nout:
        which = rng.choice(n - behind, nout, replace=False)
        if outlier_bias:                                                       # one-sided: they drag the first round's estimate
            px[which] += rng.uniform(2.5, 9, (nout, 2)) * sigma[which, None]
        else:
            px[which] += rng.choice([-1.0, 1.0], (nout, 2)) * rng.uniform(4, 40, (nout, 2)) * sigma[which, None]
    sc = dict(problem=p, xy=px.astype(F32), ur=np.where(mono, -1.0, ur).astype(F32), inv=(1.0 / (sigma * sigma)).astype(F32),
              pos=Xw.astype(F32), close=(z < 10.0).astype(np.uint8), truth=true, octave=lvl.astype(np.int32),
              C15=_c15(pre["C"][0], _f32(Cg), _f32(Ca)),
              depth=float(np.median(np.abs(Xc[:, 2]))) if n else 10.0, speed=float(np.linalg.norm(true["v"])))
    return sc


def _c15(C9, Cg, Ca):
    """Preintegrated::C as the reference holds it: the 9x9 of the integration, then the two random-walk blocks"""
    C = np.zeros((15, 15), F32)
    C[:9, :9], C[9:12, 9:12], C[12:, 12:] = C9, Cg, Ca
    return C


LEVEL_INV_SIGMA2 = (1.0 / ((1.2 ** np.arange(8)) * (1.2 ** np.arange(8)))).astype(F32)   # mvInvLevelSigma2 of the scenes' octaves


def write_dropin_scenes(path, scenes):
    """write_scenes plus what the host templates gather from: the octaves, mvInvLevelSigma2 and the 15x15 covariance"""
    with open(path, "wb") as f:
        f.write(np.int32(len(scenes)).tobytes())
        for sc in scenes:
            assert np.array_equal(LEVEL_INV_SIGMA2[sc["octave"]], sc["inv"])
            f.write(np.asarray(sc["problem"]).tobytes())
            for k in ("xy", "ur", "inv", "pos", "close", "octave"):
                f.write(np.ascontiguousarray(sc[k]).tobytes())
            f.write(LEVEL_INV_SIGMA2.tobytes())
            f.write(np.ascontiguousarray(sc["C15"]).tobytes())


def _origin(rng):
    bg = rng.normal(0, 1, 3)
    ba = rng.normal(0, 1, 3)
    return dict(Rwb=_rot(rng.normal(0, 0.4, 3)), twb=rng.normal(0, 2.0, 3), v=np.array([6.0, 0.5, 0.1]) + rng.normal(0, 0.5, 3),
                bg=0.01 * bg / np.linalg.norm(bg), ba=0.1 * ba / np.linalg.norm(ba))


def _prior_from(sc, r):
    """what the call leaves in pFrame->mpcpi"""
    return dict(state=r["est"], H=r["H_prior"])


def build(seed, n, form, **kw):
    """a scene of `form`; form 1 is preceded by a restated LastKeyFrame call of 60 observations that makes its prior"""
    rng = np.random.default_rng(seed)
    kf = _origin(rng)
    straddle = kw.pop("straddle", None)
    if straddle:
        return _straddle(build(seed, n, form, **kw), *straddle[form])
    if form == 0:
        return make_step(rng, kf, n, 0, **kw)
    first = make_step(rng, kf, 60, 0)
    r = optimize(first)
    prior_shift = kw.pop("prior_shift", 0.0)
    pr = _prior_from(first, r)
    if prior_shift:                                                            # a prior that disagrees with the inertial edge
        pr = dict(pr, lin=dict(pr["state"], twb=pr["state"]["twb"] + prior_shift))
    return make_step(rng, first["truth"], n, 1, prior=pr, **kw)


def _straddle(sc, k, factor):
    """scales the weight of edge k.  The factor was found by bisection so that the threshold of the classification lies at the
    geometric mean of that edge's chi2 before and after the tenth update; the CPU test checks that it does."""
    inv = sc["inv"].copy()
    inv[k] = F32(float(inv[k]) * factor)
    return dict(sc, inv=inv)


CAPACITY = 2048   # msorb_pose_inertial_optimization_capacity(), checked by the GPU test
# name -> (seed, n, keywords); every scene runs in both forms unless it names one
_SCENES = {
    "n0": (11, 0, {}),
    "n5": (12, 5, {}),
    "n6": (13, 6, {}),
    "n7": (14, 7, {}),
    "n29_recover": (15, 29, dict(outliers=0.2)),
    "n29_recover_recinit": (15, 29, dict(outliers=0.2, rec_init=1)),
    "n255": (16, 255, dict(outliers=0.1)),
    "n256": (17, 256, dict(outliers=0.1)),
    "n257": (18, 257, dict(outliers=0.1)),
    "capacity": (19, CAPACITY, dict(outliers=0.05)),
    "capacity_plus_1": (20, CAPACITY + 1, dict(outliers=0.05)),
    "all_mono": (21, 120, dict(mono_frac=1.0, outliers=0.1)),
    "all_stereo": (22, 120, dict(mono_frac=0.0, outliers=0.1)),
    "mixed": (23, 120, dict(mono_frac=0.5, outliers=0.1)),
    "close_points": (24, 150, dict(mono_frac=1.0, close_frac=0.6, noise_px=1.45)),
    "behind_camera": (25, 80, dict(behind=6)),
    # a weak inertial edge lets the one-sided outliers drag round one's estimate: an edge is out after round one and in at the end
    "outliers_40pct": (40, 200, dict(outliers=0.4, start=6.0, outlier_bias=True, imu_sigma=300.0)),
    # five edges run ONE round of ten robust passes, which a weak inertial edge and a far start leave short of convergence: the
    # tenth update moves the chi2 by percents, and one edge's weight is set so that its threshold lies between the two values.
    # rec_init keeps the recovery arm from clearing the flag again.
    "stale_chi2": ((115, 106), 5, dict(start=10.0, noise_px=2.5, mono_frac=0.5, imu_sigma=300.0, rec_init=1,
                                       straddle=((1, 2.2541885375976562), (0, 1.2614798545837402)))),
    "far_start": (28, 150, dict(start=15.0, outliers=0.1)),
}
_FORM_ONLY = {"huber_prior": (1, (29, 100, dict(prior_shift=0.05))), "solver_fails": (0, (30, 40, dict(bad_info=True)))}


def scene_names():
    names = [(k, f) for k in _SCENES for f in (0, 1)]
    names += [(k, f) for k, (f, _) in _FORM_ONLY.items()]
    return tuple("%s/%d" % kf for kf in names)


GPU_SCENES = scene_names()


@functools.lru_cache(maxsize=None)
def scene(name):
    key, form = name.split("/")
    form = int(form)
    seed, n, kw = _SCENES[key] if key in _SCENES else _FORM_ONLY[key][1]
    return build(seed[form] if isinstance(seed, tuple) else seed, n, form, **dict(kw))


@functools.lru_cache(maxsize=None)
def reference(name, variant=VARIANTS[0]):
    return optimize(scene(name), variant)


@functools.lru_cache(maxsize=None)
def chain3():
    """a LastKeyFrame call whose result feeds a LastFrame call, whose result feeds a second one: the three scenes, each built on the
    RESTATEMENT's previous output"""
    rng = np.random.default_rng(31)
    kf = _origin(rng)
    a = make_step(rng, kf, 150, 0, outliers=0.1)
    ra = optimize(a)
    b = make_step(rng, a["truth"], 150, 1, prior=_prior_from(a, ra), outliers=0.1)
    rb = optimize(b)
    c = make_step(rng, b["truth"], 150, 1, prior=_prior_from(b, rb), outliers=0.1)
    return (a, b, c)


# ------------------------------------------------------------------------------------------------ comparison
def differences(a, b, sc):
    """per quantity the largest difference between two results (dicts as optimize returns)"""
    d = {}
    d["Rwb"] = float(np.abs(a["est"]["Rwb"] - b["est"]["Rwb"]).max())
    d["twb"] = float(np.abs(a["est"]["twb"] - b["est"]["twb"]).max() / sc["depth"])
    d["v"] = float(np.abs(a["est"]["v"] - b["est"]["v"]).max() / max(sc["speed"], 1e-3))
    d["bg"] = float(np.abs(a["est"]["bg"] - b["est"]["bg"]).max())
    d["ba"] = float(np.abs(a["est"]["ba"] - b["est"]["ba"]).max())
    for k in ("H_raw", "H_prior"):
        A, B = np.asarray(a[k]), np.asarray(b[k])
        d[k] = float(np.abs(A - B).max() / max(np.abs(A).max(), 1e-300))
    if "chi2_final" in a and "chi2_final" in b and "chi2" not in b:            # the host program: the edges' final chi2
        (x, t), (y, u) = a["chi2_final"], b["chi2_final"]
        t = t if t is not None else u if u is not None else 0.0
        d["chi2"] = float((np.abs(x - y) / np.maximum(np.maximum(x, y), t)).max()) if len(x) else 0.0
    if "chi2" in a and "chi2" in b and len(a["chi2"]) == len(b["chi2"]):
        d["chi2"] = max([float((np.abs(x[0] - y[0]) / np.maximum(np.maximum(x[0], y[0]), x[1])).max()) if len(x[0]) else 0.0
                         for x, y in zip(a["chi2"], b["chi2"])] + [0.0])
    return d


def decisions(r):
    """what must be equal between any two statements of the routine"""
    return (tuple(bool(f) for f in r["flags"]), int(r["n_bad"]), int(r["n_inliers"]), tuple(int(i) for i in r["iterations"]),
            tuple(int(i) for i in r["solve_failed"]))


def chi2_margin(r):
    """the smallest relative distance of a compared chi2 to its threshold"""
    m = [float((np.abs(c - t) / t).min()) for c, t in r["chi2"] if len(c)]
    return min(m) if m else float("inf")


def threshold_margins(r):
    """the singular value nearest to 1e-6 and the eigenvalue nearest to 1e-12, as the factor between them"""
    def nearest(vals, thr):
        vals = np.abs(np.asarray(vals))
        vals = vals[vals > 0]
        return float(np.exp(np.abs(np.log(vals / thr)).min())) if len(vals) else float("inf")
    return nearest(r["sigma"], 1e-6), nearest(r["eigs"], 1e-12)


def as_result(rec, flags, sigma=None, eigs=None, form=0, chi2=None):
    """a RESULT_DTYPE record (the library's or the host program's) as optimize's dict.  chi2: the edges' final chi2, which only the
    host program writes; the library's record has none, so differences() compares no chi2 for the device"""
    N = 30 if form == 1 else 15
    e = rec["est"]
    extra = {} if chi2 is None else dict(chi2_final=(np.asarray(chi2, F64), None))
    return dict(**extra, est=dict(Rwb=e["Rwb"].reshape(3, 3), twb=e["twb"], v=e["v"], bg=e["bg"], ba=e["ba"]), flags=np.asarray(flags, bool),
                n_bad=int(rec["n_bad"]), n_inliers=int(rec["n_inliers"]), iterations=[int(i) for i in rec["iterations"]],
                solve_failed=[int(i) for i in rec["solve_failed"]], H_raw=rec["H_raw"][:N * N].reshape(N, N),
                H_prior=rec["H_prior"].reshape(15, 15), sigma=sigma if sigma is not None else np.zeros(15),
                eigs=eigs if eigs is not None else np.zeros(15))


def write_scenes(path, scenes):
    with open(path, "wb") as f:
        f.write(np.int32(len(scenes)).tobytes())
        for sc in scenes:
            f.write(np.asarray(sc["problem"]).tobytes())
            for k in ("xy", "ur", "inv", "pos", "close"):
                f.write(np.ascontiguousarray(sc[k]).tobytes())


def read_results(path, scenes):
    out = []
    with open(path, "rb") as f:
        for sc in scenes:
            n = int(sc["problem"]["n"])
            rec = np.frombuffer(f.read(RESULT_DTYPE.itemsize), RESULT_DTYPE)[0]
            flags = np.frombuffer(f.read(n), np.uint8).astype(bool)
            chi2 = np.frombuffer(f.read(8 * n), F64)
            sigma = np.frombuffer(f.read(120), F64)
            eigs = np.frombuffer(f.read(120), F64)
            out.append((rec, as_result(rec, flags, sigma, eigs, int(sc["problem"]["form"]), chi2)))
    return out


def flat(scenes):
    """the flat arrays of msorb.pose_inertial_optimization_batch"""
    pr = np.array([sc["problem"] for sc in scenes], PROBLEM_DTYPE)
    cat = lambda k, shape: (np.concatenate([sc[k].reshape(shape) for sc in scenes]) if scenes else np.zeros(shape))  # noqa: E731
    return pr, cat("xy", (-1, 2)), cat("ur", (-1,)), cat("inv", (-1,)), cat("pos", (-1, 3)), cat("close", (-1,))


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def bounds():
    return {k: MARGIN * v for k, v in golden()["D"].items()}


def within(d, b):
    return all(d[k] <= b[k] for k in d if k in b)


def measure(names=GPU_SCENES):
    """D per quantity over the scenes and the variants, the margins, and whether every variant takes the same decisions"""
    D = {k: 0.0 for k in QUANTITIES}
    margin, sv, ev, agree = float("inf"), float("inf"), float("inf"), True
    scenes = [(nm, scene(nm)) for nm in names] + [("chain3/%d" % i, sc) for i, sc in enumerate(chain3())]
    for nm, sc in scenes:
        base = optimize(sc, VARIANTS[0])
        for var in VARIANTS:
            r = base if var == VARIANTS[0] else optimize(sc, var)
            if decisions(r) != decisions(base):
                agree = False
                print("decisions differ:", nm, var)
                continue
            for k, v in differences(base, r, sc).items():
                D[k] = max(D[k], v)
            margin = min(margin, chi2_margin(r))
            s, e = threshold_margins(r)
            sv, ev = min(sv, s), min(ev, e)
    return dict(D=D, chi2_margin=margin, singular_value_factor=sv, eigenvalue_factor=ev, variants_agree=agree, margin=MARGIN,
                variants=[list(v) for v in VARIANTS], scenes=[nm for nm, _ in scenes])


if __name__ == "__main__":
    if "--measure" in sys.argv:
        m = measure()
        with open(GOLDEN, "w") as f:
            json.dump(m, f, indent=1, sort_keys=True)
        print(json.dumps(m, indent=1, sort_keys=True))
