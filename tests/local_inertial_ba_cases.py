"""Optimizer::LocalInertialBA (src/Optimizer.cc:2431-2973) after its gathering loops, restated in float64 / float32 numpy for pinhole
KeyFrames without a second camera: EdgeMono / EdgeStereo (include/G2oTypes.h:342-388, :425-493, src/G2oTypes.cc:349-373, :397-427)
over ImuCamPose (G2oTypes.cc:73-119, :192-220) and the points, EdgeInertial (G2oTypes.cc:492-594), EdgeGyroRW / EdgeAccRW
(G2oTypes.h:635-704), g2o's Levenberg with setUserLambdaInit (optimization_algorithm_levenberg.cpp:61-195), the Schur complement
of BlockSolverX (block_solver.hpp:354-486), the classification of :2876-2904 and the FAIL rule of :2911; the scene generator and
the scene list of the CPU and GPU tests.  No GPU, no library and no code shared with ms-slam_amd/csrc/local_inertial_ba_device.h:
the visual edges are evaluated in array passes, the multi-edges as whole 9x24 matrices, the system is one dense matrix over all
unknowns' pose part with the points in [P, 3, 3] blocks.  The SO3 functions, the float32 preintegration and the ordered sums are
those of tests/inertial_opt_cases.py, EdgeInertial and the state update those of tests/pose_inertial_cases.py.

TWO states at the end: the reference calls chi2() without computeError(), so err_end and every edge's chi2 of the classification
are those of the state the LAST TRIAL wrote, accepted or not; isDepthPositive() reads the restored estimate (`stale=False` gives
what a routine that re-evaluated at the estimate would return).

The variants that measure what the reference leaves to Eigen / libm (`python tests/local_inertial_ba_cases.py --measure` writes
tests/golden/local_inertial_ba_sensitivity.json):
  * `sum_order`: how the edges' terms are added into the vertices' blocks, the points' terms into the Schur complement, the
    products of the multi-edges' quadratic forms and the costs: 'forward', 'reverse', 'pairwise' (numpy's sum and matmul);
  * `solver`: 'ldlt' (unpivoted square-root-free L D L^T, the point blocks inverted by cofactors) or 'lapack';
  * `nudge`: sin, cos, acos and their float32 forms one ulp up; `ortho`: NormalizeRotation by SVD or by Newton's polar iteration.
The first of VARIANTS is THE restatement.
"""
import functools
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from inertial_opt_cases import DBL_MAX, EDGE_DTYPE, F32, F64, _rot, mm, mv, ordered_sum  # noqa: E402
import pose_inertial_cases as pic  # noqa: E402

MARGIN = 16                        # the project's margin over the measured spread (DESIGN.md sections 9 to 20)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_inertial_ba_sensitivity.json")
VARIANTS = (("forward", "ldlt", False, "svd"), ("reverse", "ldlt", False, "svd"), ("pairwise", "ldlt", False, "svd"),
            ("forward", "lapack", False, "svd"), ("forward", "ldlt", True, "svd"), ("forward", "ldlt", False, "polar"))
#            (sum_order, solver, nudge, ortho)
QUANTITIES = ("Rwb", "twb", "v", "bg", "ba", "points", "chi2", "cost")
CAPACITY = 25                      # msorb_local_inertial_ba_capacity(), checked by the GPU test

PROBLEM_DTYPE = np.dtype([("large", "<i4"), ("iterations", "<i4"), ("reserved", "<i4", 2)])
KF_DTYPE = np.dtype([("Rwb", "<f8", 9), ("twb", "<f8", 3), ("v", "<f8", 3), ("bg", "<f8", 3), ("ba", "<f8", 3), ("Rcw", "<f8", 9),
                     ("tcw", "<f8", 3), ("Rcb", "<f8", 9), ("tcb", "<f8", 3), ("tbc", "<f8", 3), ("fx", "<f4"), ("fy", "<f4"),
                     ("cx", "<f4"), ("cy", "<f4"), ("mbf", "<f4"), ("kind", "<i4")])
IEDGE_DTYPE = np.dtype([("pre", EDGE_DTYPE), ("info_gyro", "<f8", 9), ("info_acc", "<f8", 9), ("huber", "<i4"), ("downweight", "<i4")])
KF_OUT_DTYPE = np.dtype([("Rwb", "<f8", 9), ("twb", "<f8", 3), ("Rcw", "<f8", 9), ("tcw", "<f8", 3), ("v", "<f8", 3), ("bg", "<f8", 3),
                         ("ba", "<f8", 3), ("Rcw_f", "<f4", 9), ("tcw_f", "<f4", 3), ("v_f", "<f4", 3), ("bias_f", "<f4", 6),
                         ("reserved_f", "<f4")])
RESULT_DTYPE = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("trials", "<i4"), ("rejected_trials", "<i4"), ("n_outliers", "<i4"),
                         ("reserved", "<i4"), ("chi2_initial", "<f8"), ("chi2_final", "<f8"), ("lambda_final", "<f8"), ("err", "<f4"),
                         ("err_end", "<f4")])
assert (PROBLEM_DTYPE.itemsize, KF_DTYPE.itemsize, IEDGE_DTYPE.itemsize, KF_OUT_DTYPE.itemsize, RESULT_DTYPE.itemsize) == (16, 408, 1080, 352, 56)

CHI2_MONO, CHI2_STEREO = F32(5.991), F32(7.815)                                # :2433-2434 as floats
CHI2_CLOSE = F32(1.5) * CHI2_MONO                                              # :2884
D_MONO, D_STEREO, D_INERTIAL = float(F32(math.sqrt(5.991))), float(F32(math.sqrt(7.815))), math.sqrt(16.92)


# ------------------------------------------------------------------------------------------------ the state
def initial_state(sc):
    """VertexPose(pKF) / VertexVelocity / VertexGyroBias / VertexAccBias of every KeyFrame, the points widened"""
    st = []
    for k in sc["kf"]:
        st.append(dict(Rwb=k["Rwb"].reshape(3, 3).astype(F64), twb=k["twb"].astype(F64), v=k["v"].astype(F64), bg=k["bg"].astype(F64),
                       ba=k["ba"].astype(F64), Rcw=k["Rcw"].reshape(3, 3).astype(F64), tcw=k["tcw"].astype(F64), its=0))
    return st, sc["pos"].astype(F64)


def _scatter(values, target, size, order):
    """sum of values[i] into out[target[i]] in the given order of i"""
    out = np.zeros((size,) + values.shape[1:])
    if order == "pairwise":
        srt = np.argsort(target, kind="stable")
        t, v = target[srt], values[srt]
        cut = np.flatnonzero(np.diff(t)) + 1
        for lo, hi in zip(np.concatenate([[0], cut]), np.concatenate([cut, [len(t)]])):
            if hi > lo:
                out[t[lo]] = np.sum(v[lo:hi], axis=0)
        return out
    idx = np.arange(len(target)) if order == "forward" else np.arange(len(target))[::-1]
    np.add.at(out, target[idx], values[idx])
    return out


# ------------------------------------------------------------------------------------------------ the visual edges
def visual_errors(sc, st, pts):
    """computeError of both edges -> e [E, 3] (e[:, 2] = 0 for a mono edge), Xc [E, 3], chi2 [E]"""
    kf, ek, ep = sc["kf"], sc["edge_kf"], sc["edge_pt"]
    Rcw = np.stack([s["Rcw"] for s in st])[ek] if len(st) else np.zeros((0, 3, 3))
    tcw = np.stack([s["tcw"] for s in st])[ek] if len(st) else np.zeros((0, 3))
    fx, fy, cx, cy, bf = (kf[k].astype(F64)[ek] for k in ("fx", "fy", "cx", "cy", "mbf"))
    Xc = mv(Rcw, pts[ep]) + tcw
    w = sc["inv"].astype(F64)
    stereo = sc["ur"] >= 0
    with np.errstate(divide="ignore", invalid="ignore"):
        p0 = (fx * Xc[:, 0]) / Xc[:, 2] + cx
        p1 = (fy * Xc[:, 1]) / Xc[:, 2] + cy
        e = np.zeros((len(ek), 3))
        e[:, 0] = sc["xy"][:, 0].astype(F64) - p0
        e[:, 1] = sc["xy"][:, 1].astype(F64) - p1
        e[:, 2] = np.where(stereo, sc["ur"].astype(F64) - (p0 - bf * (1 / Xc[:, 2])), 0.0)
    c2 = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
    return e, Xc, np.where(stereo, c2 + e[:, 2] * (w * e[:, 2]), c2)


def visual_jacobians(sc, st, Xc):
    """linearizeOplus (G2oTypes.cc:349-373, :397-427) -> Ja [E, 3, 3] = -proj_jac Rcw, Jb [E, 3, 6] = (proj_jac Rcb) SE3deriv(Xb)"""
    kf, ek = sc["kf"], sc["edge_kf"]
    n = len(ek)
    Rcw = np.stack([s["Rcw"] for s in st])[ek] if len(st) else np.zeros((0, 3, 3))
    Rcb, tbc = kf["Rcb"].reshape(-1, 3, 3)[ek], kf["tbc"][ek]
    fx, fy, bf = (kf[k].astype(F64)[ek] for k in ("fx", "fy", "mbf"))
    stereo = sc["ur"] >= 0
    Xb = mv(np.swapaxes(Rcb, 1, 2), Xc) + tbc
    zz = Xc[:, 2] * Xc[:, 2]
    pj = np.zeros((n, 3, 3))
    pj[:, 0, 0] = fx / Xc[:, 2]
    pj[:, 0, 2] = (-fx * Xc[:, 0]) / zz
    pj[:, 1, 1] = fy / Xc[:, 2]
    pj[:, 1, 2] = (-fy * Xc[:, 1]) / zz
    pj[:, 2, 0] = np.where(stereo, pj[:, 0, 0], 0.0)
    pj[:, 2, 2] = np.where(stereo, pj[:, 0, 2] + bf * (1.0 / zz), 0.0)
    Ja = -mm(pj, Rcw)
    M = mm(pj, Rcb)
    D = np.zeros((n, 3, 6))
    x, y, z = Xb[:, 0], Xb[:, 1], Xb[:, 2]
    D[:, 0, 1], D[:, 0, 2], D[:, 1, 0], D[:, 1, 2], D[:, 2, 0], D[:, 2, 1] = z, -y, -z, x, y, -x
    D[:, 0, 3] = D[:, 1, 4] = D[:, 2, 5] = 1.0
    Jb = (M[:, :, 0, None] * D[:, None, 0, :] + M[:, :, 1, None] * D[:, None, 1, :]) + M[:, :, 2, None] * D[:, None, 2, :]
    return Ja, Jb


def _huber(chi2, delta, robust=True):
    """RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91) -> rho[0], rho[1]"""
    chi2 = np.asarray(chi2, F64)
    lin = (chi2 > delta * delta) & robust
    sq = np.sqrt(np.where(lin, chi2, 1.0))
    return np.where(lin, (2 * sq) * delta - delta * delta, chi2), np.where(lin, delta / sq, 1.0)


def _quad(A, wr, B):
    """sum over the error's rows of (A^T wr) B per edge: [E, a, b]"""
    return ((A[:, 0, :, None] * wr) * B[:, 0, None, :] + (A[:, 1, :, None] * wr) * B[:, 1, None, :]) + (A[:, 2, :, None] * wr) * B[:, 2, None, :]


# ------------------------------------------------------------------------------------------------ the inertial edges
def _iedge_info(E):
    info = E["pre"]["info"].reshape(9, 9)
    return info * 1e-2 if int(E["downweight"]) else info                       # :2665


def inertial_edges(sc, st, free_of, nudge, ortho, jac):
    """per active inertial edge (e9, J [9, 24] or None, chi2, rho0, rho1, eg, ea)"""
    out = []
    for E in sc["ie"]:
        a, b = int(E["pre"]["kf_prev"]), int(E["pre"]["kf_cur"])
        if free_of[a] < 0 and free_of[b] < 0:                                  # all vertices fixed: not active
            out.append(None)
            continue
        e, J = pic.inertial_edge(dict(problem=dict(pre=E["pre"])), st[b], st[a], nudge, ortho, jac)
        info = _iedge_info(E)
        chi = float(e @ (info @ e))
        rho0, rho1 = _huber(chi, D_INERTIAL, bool(E["huber"]))
        out.append((e, J, chi, float(rho0), float(rho1), st[b]["bg"] - st[a]["bg"], st[b]["ba"] - st[a]["ba"]))
    return out


def total_cost(sc, chi2, iedges, order):
    """activeRobustChi2: the visual edges' rho, then per inertial edge EdgeInertial's rho, EdgeGyroRW's and EdgeAccRW's chi2"""
    stereo = sc["ur"] >= 0
    rho0, _ = _huber(chi2, np.where(stereo, D_STEREO, D_MONO))
    c = float(ordered_sum(rho0, order)) if len(rho0) else 0.0
    for E, t in zip(sc["ie"], iedges):
        if t is None:
            continue
        _, _, _, r0, _, eg, ea = t
        c += r0
        c += float(eg @ (E["info_gyro"].reshape(3, 3) @ eg))
        c += float(ea @ (E["info_acc"].reshape(3, 3) @ ea))
    return c


# ------------------------------------------------------------------------------------------------ the system
def unknowns(sc):
    """free_of [K], and per free KeyFrame the indices of its fifteen unknowns: poses first (g2o orders by vertex id), then
    velocity, gyro bias, acc bias per KeyFrame"""
    kind = sc["kf"]["kind"]
    free = np.flatnonzero(kind == 0)
    free_of = np.full(len(kind), -1)
    free_of[free] = np.arange(len(free))
    Kf = len(free)
    idx = [np.concatenate([6 * i + np.arange(6), 6 * Kf + 9 * i + np.arange(9)]) for i in range(Kf)]
    return free, free_of, idx


def linearise(sc, st, pts, variant):
    """buildSystem at the state -> dict(H [n, n] symmetric, b [n], Hll [P, 3, 3], bl [P, 3], W [E, 6, 3] (zero for a fixed
    KeyFrame), cost, chi2 [E], iedges)"""
    order, solver, nudge, ortho = variant
    free, free_of, idx = unknowns(sc)
    Kf, n, P = len(free), 15 * len(free), len(pts)
    ek, ep = sc["edge_kf"], sc["edge_pt"]
    e, Xc, chi2 = visual_errors(sc, st, pts)
    stereo = sc["ur"] >= 0
    _, rho1 = _huber(chi2, np.where(stereo, D_STEREO, D_MONO))
    Ja, Jb = visual_jacobians(sc, st, Xc)
    w = sc["inv"].astype(F64)
    wr = (rho1 * w)[:, None, None]
    omr = (-(w[:, None] * e)) * rho1[:, None]
    Hll = _scatter(_quad(Ja, wr, Ja), ep, P, order)
    bl = _scatter((Ja[:, 0, :] * omr[:, 0, None] + Ja[:, 1, :] * omr[:, 1, None]) + Ja[:, 2, :] * omr[:, 2, None], ep, P, order)
    fe = free_of[ek]
    on = fe >= 0
    Hpp = _scatter(_quad(Jb, wr, Jb)[on], fe[on], Kf, order)
    bp = _scatter(((Jb[:, 0, :] * omr[:, 0, None] + Jb[:, 1, :] * omr[:, 1, None]) + Jb[:, 2, :] * omr[:, 2, None])[on], fe[on], Kf, order)
    W = np.where(on[:, None, None], _quad(Jb, wr, Ja), 0.0)
    H, b = np.zeros((n, n)), np.zeros(n)
    for i in range(Kf):
        H[6 * i:6 * i + 6, 6 * i:6 * i + 6] = Hpp[i]
        b[6 * i:6 * i + 6] = bp[i]
    ied = inertial_edges(sc, st, free_of, nudge, ortho, True)
    seq = range(len(ied)) if order != "reverse" else range(len(ied) - 1, -1, -1)
    for m in seq:
        if ied[m] is None:
            continue
        E = sc["ie"][m]
        ee, J, chi, _, r1, eg, ea = ied[m]
        a, c = int(E["pre"]["kf_prev"]), int(E["pre"]["kf_cur"])
        Hm, bm = pic.quadratic(J, r1 * _iedge_info(E), ee, order)             # robustInformation: rho' omega, and rho' omega e
        cols = np.full(24, -1)
        if free_of[a] >= 0:
            cols[0:15] = idx[free_of[a]]
        if free_of[c] >= 0:
            cols[15:24] = idx[free_of[c]][:9]
        sel = cols >= 0
        H[np.ix_(cols[sel], cols[sel])] += Hm[np.ix_(sel, sel)]
        b[cols[sel]] += bm[sel]
        for info, lo, err in ((E["info_gyro"].reshape(3, 3), 9, eg), (E["info_acc"].reshape(3, 3), 12, ea)):
            Oe = mv(info, err)
            ia = idx[free_of[a]][lo:lo + 3] if free_of[a] >= 0 else None
            ic = idx[free_of[c]][lo:lo + 3] if free_of[c] >= 0 else None
            if ia is not None:
                H[np.ix_(ia, ia)] += info
                b[ia] += Oe
            if ic is not None:
                H[np.ix_(ic, ic)] += info
                b[ic] += -Oe
            if ia is not None and ic is not None:
                H[np.ix_(ia, ic)] += -info
                H[np.ix_(ic, ia)] += -info.T
    return dict(H=H, b=b, Hll=Hll, bl=bl, W=W, chi2=chi2, iedges=ied, cost=total_cost(sc, chi2, ied, order))


def _inv3(M):
    """Eigen's 3x3 inverse: cofactors times 1 / det, det along the first column, of the symmetric M read from its upper triangle"""
    m00, m01, m02, m11, m12, m22 = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]
    c00, c10, c20 = m11 * m22 - m12 * m12, m12 * m02 - m22 * m01, m01 * m12 - m02 * m11
    inv = 1.0 / ((c00 * m00 + c10 * m01) + c20 * m02)
    out = np.zeros_like(M)
    out[:, 0, 0], out[:, 0, 1], out[:, 0, 2] = c00 * inv, c10 * inv, c20 * inv
    out[:, 1, 1], out[:, 1, 2], out[:, 2, 2] = (m22 * m00 - m02 * m02) * inv, (m02 * m01 - m00 * m12) * inv, (m00 * m11 - m01 * m01) * inv
    out[:, 1, 0], out[:, 2, 0], out[:, 2, 1] = out[:, 0, 1], out[:, 0, 2], out[:, 1, 2]
    return out


def solve_trial(sc, L, lam, variant, x_prev):
    """setLambda, the Schur complement, the reduced solve and the points' back substitution -> (x [n], xl [P, 3], solved)"""
    order, solver, _, _ = variant
    free, free_of, idx = unknowns(sc)
    Kf, n, P = len(free), 15 * len(free), len(L["Hll"])
    ek, ep = sc["edge_kf"], sc["edge_pt"]
    D = L["Hll"] + lam * np.eye(3)[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        Dinv = _inv3(D) if solver == "ldlt" else (np.linalg.inv(D) if P else D)
    fe = free_of[ek]
    on = np.flatnonzero(fe >= 0)
    Wd = np.zeros((P, 6 * Kf, 3))                                              # Hpl, dense per point
    for r in range(6):
        Wd[ep[on], 6 * fe[on] + r, :] = L["W"][on, r, :]
    Yd = np.einsum("pak,pkl->pal", Wd, Dinv)
    S = L["H"] + lam * np.eye(n)
    bs = L["b"].copy()
    if P and Kf:
        S[:6 * Kf, :6 * Kf] -= ordered_sum(np.einsum("pak,pbk->pab", Yd, Wd), order)
        bs[:6 * Kf] -= ordered_sum(np.einsum("pak,pk->pa", Yd, L["bl"]), order)
    sol = pic.solve(np.triu(S), bs, solver) if n else np.zeros(0)
    solved = sol is not None
    x = sol if solved else x_prev
    cl = L["bl"] - np.einsum("pak,a->pk", Wd, x[:6 * Kf]) if Kf else L["bl"]
    xl = np.einsum("pkl,pl->pk", Dinv, cl)
    return x, xl, solved


def apply_update(sc, st, pts, x, xl, variant):
    """push + update: a copy of the state moved by x, the ImuCamPose counters included"""
    _, _, nudge, ortho = variant
    free, _, idx = unknowns(sc)
    new = [dict(s) for s in st]
    for i, k in enumerate(free):
        K = sc["kf"][k]
        pic._update(new[k], x[idx[i]], K["Rcb"].reshape(3, 3), K["tcb"], nudge, ortho)
    return new, pts + xl


def optimize(sc, variant=VARIANTS[0], stale=True, trace=None):
    """One call -> dict(status, iterations, trials, rejected_trials, chi2_initial, chi2_final, lambda_final, err, err_end, st (the
    KeyFrames' estimates), pts, flags, n_outliers, chi2 (every visual edge's chi2 as the classification reads it), thr (its
    threshold), flags_at_estimate (what a classification at the returned estimate would flag))"""
    order = variant[0]
    large = bool(sc["large"])
    max_it = int(sc["iterations"]) if int(sc["iterations"]) > 0 else (4 if large else 10)
    free, free_of, idx = unknowns(sc)
    E = len(sc["edge_kf"])
    st, pts = initial_state(sc)
    if len(free) == 0 and E == 0:
        return dict(status=2, iterations=0, trials=0, rejected_trials=0, chi2_initial=0.0, chi2_final=0.0, lambda_final=0.0, st=st, pts=pts,
                    flags=np.zeros(0, bool), n_outliers=0, chi2=np.zeros(0), thr=np.zeros(0), err=F32(0), err_end=F32(0),
                    flags_at_estimate=np.zeros(0, bool), decision_margin=float("inf"))
    n = 15 * len(free)
    lam, ni, n_bad, ok = 0.0, 2.0, 0, True
    iterations = trials = rejected = 0
    dmargin = float("inf")
    x = np.zeros(n)
    chi2_initial = chi2_end = None
    last_chi2 = None
    for it in range(max_it):
        if not ok:
            break
        L = linearise(sc, st, pts, variant)
        current = ini = L["cost"]
        last_chi2, chi2_end = L["chi2"], current
        if it == 0:
            chi2_initial = current
            lam, ni, n_bad = (1e-2 if large else 1e0), 2.0, 0                  # setUserLambdaInit (:2547-2555)
        rho, qmax = 0.0, 0
        while True:
            x, xl, solved = solve_trial(sc, L, lam, variant, x)
            st2, pts2 = apply_update(sc, st, pts, x, xl, variant)
            _, _, c2 = visual_errors(sc, st2, pts2)
            ied = inertial_edges(sc, st2, free_of, variant[2], variant[3], False)
            temp = total_cost(sc, c2, ied, order)
            last_chi2, chi2_end = c2, temp
            if not solved:
                temp = DBL_MAX
            scale = 0.0
            for i in range(len(free)):
                for j in idx[i]:
                    scale += x[j] * (lam * x[j] + L["b"][j])
            scale += float(ordered_sum((xl * (lam * xl + L["bl"])).reshape(-1), "forward")) if len(pts) else 0.0
            rho = (current - temp) / (scale + 1e-3)
            trials += 1
            dmargin = min(dmargin, abs(current - temp) / max(current, 1.0))
            if trace is not None:
                trace.append(dict(it=it, lam=lam, rho=rho, temp=temp, current=current))
            if rho > 0 and math.isfinite(temp):
                y = 2 * rho - 1
                alpha = min(1.0 - (y * y) * y, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                current = temp
                st, pts = st2, pts2
            else:
                lam *= ni
                ni *= 2
                rejected += 1
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        iterations += 1
        if qmax == 10 or rho == 0:
            ok = False
            continue
        n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
        if n_bad >= 3:
            ok = False
    if chi2_initial is None:
        _, _, last_chi2 = visual_errors(sc, st, pts)
        chi2_initial = chi2_end = total_cost(sc, last_chi2, inertial_edges(sc, st, free_of, variant[2], variant[3], False), order)
    # ---- the classification (:2876-2904)
    _, _, at_est = visual_errors(sc, st, pts)
    stereo = sc["ur"] >= 0
    close = sc["close"].astype(bool)[sc["edge_pt"]]
    thr = np.where(stereo, float(CHI2_STEREO), np.where(close, float(CHI2_CLOSE), float(CHI2_MONO)))
    Rcw = np.stack([s["Rcw"] for s in st])[sc["edge_kf"]] if E else np.zeros((0, 3, 3))
    tcw = np.stack([s["tcw"] for s in st])[sc["edge_kf"]] if E else np.zeros((0, 3))
    X = pts[sc["edge_pt"]]
    depth_ok = ((Rcw[:, 2, 0] * X[:, 0] + Rcw[:, 2, 1] * X[:, 1]) + Rcw[:, 2, 2] * X[:, 2]) + tcw[:, 2] > 0.0
    used = last_chi2 if stale else at_est
    flags = (used > thr) | (~stereo & ~depth_ok)
    flags_at = (at_est > thr) | (~stereo & ~depth_ok)
    err, err_end = F32(chi2_initial), F32(chi2_end)
    with np.errstate(over="ignore"):
        fail = (F32(2) * err < err_end or np.isnan(err) or np.isnan(err_end)) and not large   # :2911
    return dict(status=1 if fail else 0, iterations=iterations, trials=trials, rejected_trials=rejected, chi2_initial=chi2_initial,
                chi2_final=chi2_end, lambda_final=lam, err=err, err_end=err_end, st=st, pts=pts, flags=flags, n_outliers=int(flags.sum()),
                chi2=used, thr=thr, flags_at_estimate=flags_at, decision_margin=dmargin)


# ------------------------------------------------------------------------------------------------ scenes
def _kf_record(rec, Rwb, twb, v, bg, ba, kind):
    rec["Rwb"], rec["twb"], rec["v"], rec["bg"], rec["ba"], rec["kind"] = np.asarray(Rwb).reshape(9), twb, v, bg, ba, kind
    rec["Rcw"] = pic._f32(pic.RCB @ np.asarray(Rwb).T).reshape(9)              # GetPose() widened
    rec["tcw"] = pic._f32(pic.RCB @ (-np.asarray(Rwb).T @ twb) + pic.TCB)
    rec["Rcb"], rec["tcb"], rec["tbc"] = pic.RCB.reshape(9), pic.TCB, pic._f32(-pic.RCB.T @ pic.TCB)
    for k, val in pic.KITTI.items():
        rec[k] = val


def build(seed, n_free, n_points, n_fixed=2, prev=True, mono_frac=0.3, outliers=0.0, noise_px=0.6, start=1.0, point_noise=0.01,
          obs_frac=0.8, large=False, iterations=0, rec_init=False, close_frac=None, behind=0, single_obs=0, fixed_only=0,
          point_start=1.0, depth=(4.0, 40.0), max_edges=None, prev_observes=True, imu_noise=1.0, bias_start=1.0):
    """A window of n_free free KeyFrames along an inertial chain generated as pose_inertial_cases.make_step does (float32
    preintegration of noisy IMU samples, the next true state from it), preceded by the fixed KeyFrame before the window (kind 1;
    prev=False: the oldest window KeyFrame has no mPrevKF and is itself the kind 1 one, :2483-2488), n_fixed fixed observers (kind
    2), n_points points seen from the KeyFrames' true cameras.  The estimates start `start` times a small perturbation away."""
    rng = np.random.default_rng(seed)
    rng_bias = np.random.default_rng(seed + 100003)                            # the biases' start offsets: draws of their own
    truth = [pic._origin(rng)]
    links, c15 = [], []
    for _ in range(n_free if prev else max(n_free, 0)):
        step = pic.make_step(rng, truth[-1], 0, 0, sub=12, imu_noise=imu_noise)
        links.append(step["problem"])
        c15.append(step["C15"])
        truth.append(step["truth"])
    n_chain = len(truth)                                                       # chain[0] is the kind 1 KeyFrame
    K = n_chain + n_fixed
    kf = np.zeros(K, KF_DTYPE)
    true_pose = []
    for i, t in enumerate(truth):
        fixed = i == 0
        s = 0.0 if fixed else start
        Rwb0 = pic._f32(t["Rwb"] @ _rot(s * rng.normal(0, 0.004, 3)))
        twb0 = pic._f32(t["twb"] + s * rng.normal(0, 0.01, 3))
        bias_from = truth[max(i - 1, 0)]
        # a free KeyFrame's biases start away from its predecessor's, so that both bias vertices have somewhere to move
        off = 0.0 if fixed else bias_start
        _kf_record(kf[i], Rwb0, twb0, pic._f32(t["v"] + s * rng.normal(0, 0.02, 3)), pic._f32(bias_from["bg"] + off * rng_bias.normal(0, 3e-4, 3)),
                   pic._f32(bias_from["ba"] + off * rng_bias.normal(0, 3e-3, 3)), 1 if fixed else 0)
        true_pose.append((t["Rwb"], t["twb"]))
    for j in range(n_fixed):                                                   # observers beside the chain
        base = truth[rng.integers(0, n_chain)]
        Rwb = base["Rwb"] @ _rot(rng.normal(0, 0.05, 3))
        twb = base["twb"] + base["Rwb"] @ np.array([rng.normal(0, 0.3), rng.uniform(0.5, 1.5) * rng.choice([-1, 1]), rng.normal(0, 0.1)])
        Rwb, twb = pic._f32(Rwb), pic._f32(twb)
        _kf_record(kf[n_chain + j], Rwb, twb, np.zeros(3), np.zeros(3), np.zeros(3), 2)
        true_pose.append((Rwb, twb))
    ie = np.zeros(len(links), IEDGE_DTYPE)
    for i, pr in enumerate(links):
        ie[i]["pre"] = pr["pre"]
        ie[i]["pre"]["kf_prev"], ie[i]["pre"]["kf_cur"] = i, i + 1
        ie[i]["info_gyro"], ie[i]["info_acc"] = pr["info_gyro"], pr["info_acc"]
        oldest = i == 0                                                        # i == N - 1 of the reference's newest-first window (also without mPrevKF: N counts after the pop)
        ie[i]["huber"], ie[i]["downweight"] = int(oldest or rec_init), int(oldest)
    # ---- points and observations
    cams = [(pic.RCB @ R.T, pic.RCB @ (-R.T @ t) + pic.TCB) for R, t in true_pose]
    P = n_points
    src = rng.integers(0, n_chain, P)
    z = rng.uniform(depth[0], depth[1], P)
    if close_frac is not None:
        k = int(round(close_frac * P))
        z[:k], z[k:] = rng.uniform(3.0, 9.0, k), rng.uniform(12.0, 40.0, P - k)
    u, v = rng.uniform(100, 1100, P), rng.uniform(40, 330, P)
    Xc = np.stack([(u - pic.KITTI["cx"]) / pic.KITTI["fx"] * z, (v - pic.KITTI["cy"]) / pic.KITTI["fy"] * z, z], 1)
    Xw = np.stack([cams[s][0].T @ (Xc[p] - cams[s][1]) for p, s in enumerate(src)]) if P else np.zeros((0, 3))
    ek, ep, xy, ur, inv, octv = [], [], [], [], [], []
    lvl_all = rng.integers(0, 8, (P, K))
    for p in range(P):
        seen = []
        for k in range(K):
            if k == 0 and not prev_observes:
                continue
            Xk = cams[k][0] @ Xw[p] + cams[k][1]
            if Xk[2] < 1.0:
                continue
            uu = pic.KITTI["fx"] * Xk[0] / Xk[2] + pic.KITTI["cx"]
            vv = pic.KITTI["fy"] * Xk[1] / Xk[2] + pic.KITTI["cy"]
            if not (0 < uu < 1241 and 0 < vv < 376):
                continue
            seen.append((k, uu, vv, Xk[2]))
        if p >= P - fixed_only:
            seen = [s for s in seen if kf[s[0]]["kind"] != 0]
        elif p >= P - fixed_only - single_obs:
            seen = [s for s in seen if s[0] == src[p]] or seen[:1]
        else:
            keep = rng.uniform(0, 1, len(seen)) < obs_frac
            keep[[i for i, s in enumerate(seen) if s[0] == src[p]]] = True
            seen = [s for s, kp in zip(seen, keep) if kp]
        for k, uu, vv, zz in seen:
            sig = 1.2 ** lvl_all[p, k]
            mono = rng.uniform() < mono_frac
            obs = [uu + noise_px * sig * rng.normal(), vv + noise_px * sig * rng.normal()]
            right = uu - pic.KITTI["mbf"] / zz + noise_px * sig * rng.normal()
            if not mono and right < 1.0:                                       # no match in the right image: u_right < 0 means mono
                if k != src[p]:
                    continue
                right = 1.0
            ek.append(k)
            ep.append(p)
            xy.append(obs)
            ur.append(-1.0 if mono else right)
            inv.append(1.0 / (sig * sig))
            octv.append(int(lvl_all[p, k]))
    ek, ep = np.asarray(ek, np.int32), np.asarray(ep, np.int32)
    xy, ur, inv = np.asarray(xy, F64).reshape(-1, 2), np.asarray(ur, F64), np.asarray(inv, F64)
    octv = np.asarray(octv, np.int32)
    if max_edges is not None:
        ek, ep, xy, ur, inv, octv = ek[:max_edges], ep[:max_edges], xy[:max_edges], ur[:max_edges], inv[:max_edges], octv[:max_edges]
    E = len(ek)
    planted = np.zeros(E, bool)
    nout = int(round(outliers * E))
    if nout:
        which = rng.choice(E, nout, replace=False)
        xy[which] += rng.choice([-1.0, 1.0], (nout, 2)) * rng.uniform(8, 40, (nout, 2)) / np.sqrt(inv[which])[:, None]
        planted[which] = True
    pos = Xw + point_start * point_noise * np.linalg.norm(Xc, axis=1)[:, None] * rng.normal(0, 1, (P, 3)) if P else Xw
    if behind:                                                                 # mono points that start and stay behind their camera
        for p in range(behind):
            m = np.flatnonzero(ep == p)
            ur[m] = -1.0
            k = int(ek[m[0]])
            pos[p] = cams[k][0].T @ (np.array([0.3, 0.2, -6.0]) - cams[k][1])
    return dict(large=int(large), iterations=int(iterations), kf=kf, ie=ie, pos=pos.astype(F32), close=(z < 10.0).astype(np.uint8),
                edge_kf=ek, edge_pt=ep, xy=xy.astype(F32), ur=ur.astype(F32), inv=inv.astype(F32), planted=planted,
                octave=octv, C15=np.asarray(c15, F32).reshape(-1, 15, 15),
                truth=truth, true_points=Xw, depth=float(np.median(z)) if P else 10.0,
                speed=float(np.linalg.norm(truth[-1]["v"])))


# name -> (seed, n_free, n_points, keywords).  The cost has steps of about 1e-7 of its value (the preintegration's bias correction
# is float32), so once Levenberg has converged the sign of rho, and with it the number of trials, is decided by rounding, in the
# reference as here.  A scene whose counts are compared must stop before that floor (decision_margin, checked by the CPU test):
# most scenes therefore run 3 iterations, and the ones that run the reference's 10 / 4 converge slowly (outliers under Huber, points
# behind the camera, a gross start).
_SCENES = {
    "n1": (101, 1, 40, dict(iterations=3)),
    "n2": (102, 2, 40, dict(iterations=3)),
    "n3": (103, 3, 40, dict(start=3.0, iterations=3)),
    "n4": (301, 4, 40, dict(start=120.0, point_start=30.0, iterations=6)),       # six rejected trials after five accepted updates
    "n10": (105, 10, 80, dict(n_fixed=3, outliers=0.15, start=30.0)),
    "n25_large": (106, 25, 100, dict(large=True, n_fixed=3, outliers=0.15, start=30.0)),
    "no_prev": (107, 3, 40, dict(prev=False, iterations=3)),
    "rec_init": (108, 3, 40, dict(rec_init=True, iterations=3)),
    "mono_only": (109, 3, 60, dict(mono_frac=1.0, iterations=3)),
    "stereo_only": (110, 3, 40, dict(mono_frac=0.0, iterations=3)),
    "mixed": (111, 3, 40, dict(mono_frac=0.5, iterations=3)),
    "close_points": (112, 3, 80, dict(mono_frac=1.0, close_frac=0.5, noise_px=1.5, iterations=3)),
    "behind": (113, 3, 40, dict(behind=2, iterations=3)),
    "single_obs": (114, 3, 40, dict(single_obs=6, mono_frac=0.0, iterations=3)),
    "fixed_only_point": (115, 3, 40, dict(fixed_only=4, n_fixed=3, iterations=3)),
    "p65": (116, 2, 65, dict(iterations=3)),
    "p257": (117, 2, 257, dict(obs_frac=0.5, iterations=3)),
    "e1025": (118, 4, 400, dict(max_edges=1025, iterations=3)),
    "outliers": (119, 4, 80, dict(outliers=0.2, start=10.0)),
    "rejected_trials": (339, 4, 40, dict(start=120.0, point_start=30.0, iterations=6)),
    "it1": (121, 3, 40, dict(iterations=1)),
    "it3": (122, 3, 40, dict(iterations=3)),
    # exact zero residuals cannot be asked of float32 observations and states, so rho is small, not 0: one iteration, nothing moves
    "at_optimum": (123, 3, 40, dict(noise_px=0.0, start=0.0, point_noise=0.0, imu_noise=0.0, bias_start=0.0, iterations=1)),
    "realistic": (124, 10, 600, dict(n_fixed=5, outliers=0.05, start=10.0)),
}
GPU_SCENES = tuple(_SCENES)


@functools.lru_cache(maxsize=None)
def scene(name):
    seed, n_free, n_points, kw = _SCENES[name]
    return build(seed, n_free, n_points, **dict(kw))


@functools.lru_cache(maxsize=None)
def reference(name, variant=VARIANTS[0]):
    return optimize(scene(name), variant)


def zero_noise(sc):
    """the scene with exact measurements at the generator's state: an exact float32 state cannot be asked of the observations, so
    the observations are recomputed in double from the float32 state the call starts from"""
    st, pts = initial_state(sc)
    _, Xc, _ = visual_errors(sc, st, pts)
    kf, ek = sc["kf"], sc["edge_kf"]
    fx, fy, cx, cy, bf = (kf[k].astype(F64)[ek] for k in ("fx", "fy", "cx", "cy", "mbf"))
    u, v = fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy
    return dict(sc, xy=np.stack([u, v], 1).astype(F32), ur=np.where(sc["ur"] >= 0, u - bf / Xc[:, 2], -1.0).astype(F32))


# ------------------------------------------------------------------------------------------------ comparison
def differences(a, b, sc):
    """per quantity the largest difference between two results (dicts as optimize returns)"""
    d = {k: 0.0 for k in QUANTITIES}
    for s, t in zip(a["st"], b["st"]):
        d["Rwb"] = max(d["Rwb"], float(np.abs(s["Rwb"] - t["Rwb"]).max()))
        d["twb"] = max(d["twb"], float(np.abs(s["twb"] - t["twb"]).max() / sc["depth"]))
        d["v"] = max(d["v"], float(np.abs(s["v"] - t["v"]).max() / max(sc["speed"], 1e-3)))
        d["bg"] = max(d["bg"], float(np.abs(s["bg"] - t["bg"]).max()))
        d["ba"] = max(d["ba"], float(np.abs(s["ba"] - t["ba"]).max()))
    if len(a["pts"]):
        d["points"] = float(np.abs(a["pts"] - b["pts"]).max() / sc["depth"])
    if len(a["chi2"]) and len(b["chi2"]):                                       # (the library returns no per-edge chi2)
        x, y = a["chi2"], b["chi2"]
        d["chi2"] = float((np.abs(x - y) / np.maximum(np.maximum(x, y), a["thr"])).max())
    d["cost"] = max(abs(a["chi2_final"] - b["chi2_final"]) / max(a["chi2_final"], 1.0),
                    abs(a["chi2_initial"] - b["chi2_initial"]) / max(a["chi2_initial"], 1.0))
    return d


def decisions(r):
    """what must be equal between any two statements of the routine"""
    return (int(r["status"]), int(r["iterations"]), int(r["trials"]), int(r["rejected_trials"]), int(r["n_outliers"]),
            tuple(bool(f) for f in r["flags"]))


def chi2_margin(r):
    """the smallest relative distance of a compared chi2 from its threshold"""
    return float((np.abs(r["chi2"] - r["thr"]) / r["thr"]).min()) if len(r["chi2"]) else float("inf")


def movement(sc, r):
    """how far the free vertices moved from their start, per vertex type in the units of differences(): the smallest over the free
    KeyFrames (Rwb: the largest entry; twb over the depth; v over the speed; bg, ba) and over the points that have an edge"""
    st0, pts0 = initial_state(sc)
    m = {}
    free = np.flatnonzero(sc["kf"]["kind"] == 0)
    scale = dict(Rwb=1.0, twb=sc["depth"], v=max(sc["speed"], 1e-3), bg=1.0, ba=1.0)
    for q, u in scale.items():
        m[q] = min([float(np.abs(r["st"][k][q] - st0[k][q]).max() / u) for k in free] + [float("inf")])
    seen = np.zeros(len(pts0), bool)
    seen[sc["edge_pt"]] = True
    m["points"] = float((np.abs(r["pts"] - pts0).max(axis=1) / sc["depth"])[seen].min()) if seen.any() else float("inf")
    return m


def from_records(rec, kf_out, pos_d, flags, chi2=None, thr=None):
    """the library's or the host program's outputs as optimize's dict"""
    st = [dict(Rwb=k["Rwb"].reshape(3, 3), twb=k["twb"], v=k["v"], bg=k["bg"], ba=k["ba"], Rcw=k["Rcw"].reshape(3, 3), tcw=k["tcw"])
          for k in kf_out]
    return dict(status=int(rec["status"]), iterations=int(rec["iterations"]), trials=int(rec["trials"]),
                rejected_trials=int(rec["rejected_trials"]), n_outliers=int(rec["n_outliers"]), chi2_initial=float(rec["chi2_initial"]),
                chi2_final=float(rec["chi2_final"]), lambda_final=float(rec["lambda_final"]), err=rec["err"], err_end=rec["err_end"], st=st,
                pts=np.asarray(pos_d, F64).reshape(-1, 3), flags=np.asarray(flags, bool),
                chi2=np.zeros(0) if chi2 is None else np.asarray(chi2, F64), thr=np.zeros(0) if thr is None else thr)


def write_scenes(path, scenes):
    with open(path, "wb") as f:
        f.write(np.int32(len(scenes)).tobytes())
        for sc in scenes:
            f.write(np.array([sc["large"], sc["iterations"], len(sc["kf"]), len(sc["ie"]), len(sc["pos"]), len(sc["edge_kf"])], np.int32).tobytes())
            for k in ("kf", "ie", "pos", "close", "edge_kf", "edge_pt", "xy", "ur", "inv"):
                f.write(np.ascontiguousarray(sc[k]).tobytes())


def read_results(path, scenes):
    out = []
    with open(path, "rb") as f:
        for sc in scenes:
            K, P, E = len(sc["kf"]), len(sc["pos"]), len(sc["edge_kf"])
            rec = np.frombuffer(f.read(RESULT_DTYPE.itemsize), RESULT_DTYPE)[0]
            ko = np.frombuffer(f.read(K * KF_OUT_DTYPE.itemsize), KF_OUT_DTYPE)
            pts = np.frombuffer(f.read(24 * P), F64)
            flags = np.frombuffer(f.read(E), np.uint8).astype(bool)
            chi2 = np.frombuffer(f.read(8 * E), F64)
            out.append((rec, ko, from_records(rec, ko, pts, flags, chi2, reference_thresholds(sc))))
    return out


def write_dropin_scene(path, sc, rec_init=0, no_prev=0):
    """what tests/dropin_local_inertial_ba_main.cc builds its stand-in graph from: write_scenes' records plus every edge's 15 x 15
    covariance, the octaves and mvInvLevelSigma2"""
    assert np.array_equal(pic.LEVEL_INV_SIGMA2[sc["octave"]], sc["inv"])
    with open(path, "wb") as f:
        f.write(np.array([sc["large"], rec_init, no_prev, len(sc["kf"]), len(sc["ie"]), len(sc["pos"]), len(sc["edge_kf"])], np.int32).tobytes())
        for k in ("kf", "ie", "C15", "pos", "close", "edge_kf", "edge_pt", "xy", "ur", "octave"):
            f.write(np.ascontiguousarray(sc[k]).tobytes())
        f.write(pic.LEVEL_INV_SIGMA2.tobytes())


def read_dropin_result(path, sc):
    """-> (the gathered problem as a scene dict with point_ids / kf_ids, dict(ret, change, n_new_bias, kf [K] records, pts, still))"""
    K, P, E = len(sc["kf"]), len(sc["pos"]), len(sc["edge_kf"])
    with open(path, "rb") as f:
        large, its, Kg, NIg, Pg, Eg = np.frombuffer(f.read(24), np.int32)
        g = dict(large=int(large), iterations=int(its))
        g["kf"] = np.frombuffer(f.read(Kg * KF_DTYPE.itemsize), KF_DTYPE)
        g["ie"] = np.frombuffer(f.read(NIg * IEDGE_DTYPE.itemsize), IEDGE_DTYPE)
        g["pos"] = np.frombuffer(f.read(12 * Pg), F32).reshape(-1, 3)
        g["close"] = np.frombuffer(f.read(Pg), np.uint8)
        g["edge_kf"] = np.frombuffer(f.read(4 * Eg), np.int32)
        g["edge_pt"] = np.frombuffer(f.read(4 * Eg), np.int32)
        g["xy"] = np.frombuffer(f.read(8 * Eg), F32).reshape(-1, 2)
        g["ur"] = np.frombuffer(f.read(4 * Eg), F32)
        g["inv"] = np.frombuffer(f.read(4 * Eg), F32)
        g["point_ids"] = np.frombuffer(f.read(4 * Pg), np.int32)
        g["kf_ids"] = np.frombuffer(f.read(4 * Kg), np.int32)
        ret, change, n_new_bias = np.frombuffer(f.read(12), np.int32)
        kdt = np.dtype([("n_set_pose", "<i4"), ("n_set_velocity", "<i4"), ("n_set_bias", "<i4"), ("local", "<i4"), ("fixed", "<i4"),
                        ("Rcw", "<f4", 9), ("tcw", "<f4", 3), ("v", "<f4", 3), ("bias", "<f4", 6)])
        pdt = np.dtype([("n_set_pos", "<i4"), ("n_update", "<i4"), ("pos", "<f4", 3)])
        kf = np.frombuffer(f.read(K * kdt.itemsize), kdt)
        pts = np.frombuffer(f.read(P * pdt.itemsize), pdt)
        still = np.frombuffer(f.read(E), np.uint8).astype(bool)
        assert f.read() == b""
    return g, dict(ret=int(ret), change=int(change), n_new_bias=int(n_new_bias), kf=kf, pts=pts, still=still)


def reference_thresholds(sc):
    stereo = sc["ur"] >= 0
    close = sc["close"].astype(bool)[sc["edge_pt"]]
    return np.where(stereo, float(CHI2_STEREO), np.where(close, float(CHI2_CLOSE), float(CHI2_MONO)))


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def bounds():
    return {k: MARGIN * v for k, v in golden()["D"].items()}


def within(d, b):
    return all(d[k] <= b[k] for k in d if k in b)


def measure(names=GPU_SCENES):
    """D per quantity over the scenes and the variants (C is D["chi2"]), the margin, and whether every variant takes the same
    decisions"""
    D = {k: 0.0 for k in QUANTITIES}
    margin, agree, per_scene = float("inf"), True, {}
    for nm in names:
        sc = scene(nm)
        base = optimize(sc, VARIANTS[0])
        own = {}
        for var in VARIANTS[1:]:
            r = optimize(sc, var)
            if decisions(r) != decisions(base):
                agree = False
                print("decisions differ:", nm, var)
                continue
            for k, v in differences(base, r, sc).items():
                D[k] = max(D[k], v)
                own[k] = max(own.get(k, 0.0), v)
            margin = min(margin, chi2_margin(r))
        margin = min(margin, chi2_margin(base))
        per_scene[nm] = dict(decisions=list(decisions(base)[:5]), chi2_margin=chi2_margin(base), movement=movement(sc, base),
                             decision_margin=min(base["decision_margin"], 1e300), D=own)
    return dict(D=D, chi2_margin=margin, variants_agree=agree, margin=MARGIN, variants=[list(v) for v in VARIANTS], scenes=per_scene)


if __name__ == "__main__":
    if "--measure" in sys.argv:
        m = measure()
        with open(GOLDEN, "w") as f:
            json.dump(m, f, indent=1, sort_keys=True)
        print(json.dumps(m, indent=1, sort_keys=True))
