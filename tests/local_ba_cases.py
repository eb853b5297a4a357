"""Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1040-1407, pinhole KeyFrames without a second camera) restated in float64
numpy, vectorised over the edges, with the g2o pieces it runs: core/optimization_algorithm_levenberg.cpp:61-195,
core/sparse_optimizer.cpp:376-389, core/block_solver.hpp:354-486 (the Schur complement) and :564-589 (setLambda),
core/base_binary_edge.hpp:55-120 (constructQuadraticForm), types/types_six_dof_expmap.cpp:190-196,228-274,
src/OptimizableTypes.cpp:139-160.  The SE3 pieces, the ordered sums and the constants come from tests/pose_opt_cases.py.
Also the scene generator and the named scenes of the GPU tests.  No GPU, no library.

`python tests/local_ba_cases.py --measure` writes tests/golden/local_ba_sensitivity.json.

`variant` names the order of every sum over edges (a point's Hll / bl, a KeyFrame's Hpp / bp, a block pair's Schur terms, the
coefficients of bschur, the cost, computeScale):
  forward   g2o's: the edge list front to back, the landmarks ascending.  THE REFERENCE VALUE.
  reverse, pairwise   back to front; a balanced tree.
  dense     forward sums, but no Schur complement: the full (3 P + 6 Kf) system goes through the same L D L^T, the points ordered
            first (the order that keeps the fill inside the pose block; g2o's sparse Cholesky picks a fill-reducing order too).
            It measures what the elimination order alone moves.

What the restatement fixes where the reference leaves it to Eigen (ms-slam_amd/csrc/bundle_adjustment.hip does the same):
  * a product of small matrices is the plain row-by-column sum, left to right, no fused multiply-adds;
  * the products with the structural zeros of projectJac are left out;
  * D->inverse() (block_solver.hpp:389) is Eigen's 3x3 inverse: cofactors times 1 / det, det along the first column, D read
    from its upper triangle;
  * the reduced system is solved by the square-root-free L D L^T without pivoting, one reciprocal per pivot, the substitutions
    column by column (LinearSolverEigen is a sparse Cholesky with a fill-reducing order: equal up to rounding); a pivot that is
    not positive is "solver failed" and x keeps what it held.
"""
import json
import math
import os
import sys
import time

import numpy as np

import pose_opt_cases as pc
from pose_opt_cases import F32, F64, DELTA_MONO, DELTA_STEREO, DBL_MAX, rotate, normalize_rotation, oplus, ordered_sum

VARIANTS = ("forward", "reverse", "pairwise", "dense")
CHI2_MONO, CHI2_STEREO = 5.991, 7.815      # :1340, :1368: double literals compared with a float chi2


# ------------------------------------------------------------------------------------------------------------------ sums
def seg_sum(terms, seg, nseg, order):
    """terms [m, k], seg [m] ascending segment ids -> [nseg, k]: every segment's terms added in the named order"""
    terms = np.asarray(terms, F64)
    out = np.zeros((nseg, terms.shape[1]), F64)
    if len(seg) == 0:
        return out
    if order == "forward":
        np.add.at(out, seg, terms)                      # unbuffered: one element after the other
        return out
    if order == "reverse":
        np.add.at(out, seg[::-1], terms[::-1])
        return out
    assert order == "pairwise"
    val, sg = terms.copy(), np.asarray(seg).copy()
    start = np.r_[True, sg[1:] != sg[:-1]]
    pos = np.arange(len(sg)) - np.maximum.accumulate(np.where(start, np.arange(len(sg)), 0))
    while pos.max() > 0:
        even = (pos & 1) == 0
        has_next = np.r_[(sg[1:] == sg[:-1]), False]
        idx = np.nonzero(even & has_next)[0]
        val[idx] = val[idx] + val[idx + 1]
        keep = np.nonzero(even)[0]
        val, sg, pos = val[keep], sg[keep], pos[keep] >> 1
    out[sg] = val
    return out


def _order(variant):
    return variant if variant in ("reverse", "pairwise") else "forward"


# ------------------------------------------------------------------------------------------------------------------ plan
class Plan:
    """what ms-slam_amd/csrc/local_ba_plan.h builds: the by-KeyFrame lists and the block-pair lists"""

    def __init__(self, fixed, P, edge_kf, edge_pt):
        fixed = np.asarray(fixed).astype(bool)
        self.K, self.P, self.E = len(fixed), P, len(edge_kf)
        self.free_of_kf = np.where(fixed, -1, np.cumsum(~fixed) - 1)
        self.kf_of_free = np.nonzero(~fixed)[0]
        self.Kf = len(self.kf_of_free)
        self.edge_free = self.free_of_kf[edge_kf] if self.E else np.zeros(0, int)
        fe = np.nonzero(self.edge_free >= 0)[0]
        self.kf_edge = fe[np.argsort(self.edge_free[fe], kind="stable")]      # edges of free KeyFrame 0 ascending, then 1, ...
        self.kf_seg = self.edge_free[self.kf_edge]
        begin = np.searchsorted(edge_pt, np.arange(P + 1)) if self.E else np.zeros(P + 1, int)
        ent = []
        for p in range(P):
            es = range(begin[p], begin[p + 1])
            for a in es:
                i = self.edge_free[a]
                if i < 0:
                    continue
                for b in es:
                    j = self.edge_free[b]
                    if j >= i:
                        ent.append((i * self.Kf + j, a, b))
        ent = np.array(ent, np.int64).reshape(-1, 3)
        ent = ent[np.argsort(ent[:, 0], kind="stable")]
        keys = sorted(set(ent[:, 0].tolist()) | {i * self.Kf + i for i in range(self.Kf)})
        self.pair_key = np.array(keys, np.int64)
        self.pair_i, self.pair_j = self.pair_key // max(self.Kf, 1), self.pair_key % max(self.Kf, 1)
        self.pair_a, self.pair_b = ent[:, 1], ent[:, 2]
        self.pair_seg = np.searchsorted(self.pair_key, ent[:, 0])
        self.diag_pair = np.searchsorted(self.pair_key, np.arange(self.Kf) * (self.Kf + 1))


# --------------------------------------------------------------------------------------------------------------- edges
class Problem:
    def __init__(self, s):
        kf = s["kf"]
        self.cam = {k: np.asarray(kf[k], F32).astype(F64) for k in ("fx", "fy", "cx", "cy", "mbf")}   # float until used
        self.fixed = np.asarray(kf["fixed"]).astype(bool)
        self.ek, self.ep = np.asarray(s["edge_kf"], int), np.asarray(s["edge_point"], int)
        self.ox, self.oy = np.asarray(s["xy"], F64).reshape(-1, 2).T if len(self.ek) else (np.zeros(0), np.zeros(0))
        self.ur = np.asarray(s["u_right"], F64).reshape(-1)
        self.w = np.asarray(s["inv_sigma2"], F64).reshape(-1)
        self.stereo = self.ur >= 0                                  # :1246
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)   # :1190-1191 as floats
        self.E, self.P, self.K = len(self.ek), len(s["pos_w"]), len(self.fixed)
        self.plan = Plan(self.fixed, self.P, self.ek, self.ep)

    def error(self, q, t, X):
        """q [K, 4], t [K, 3], X [P, 3] -> e [E, 3], camera-frame point [E, 3], chi2 [E]"""
        with np.errstate(all="ignore"):
            qe = q[self.ek]
            p = rotate((qe[:, 0], qe[:, 1], qe[:, 2], qe[:, 3]), X[self.ep]) + t[self.ek]    # SE3Quat::map
            x, y, z = p[:, 0], p[:, 1], p[:, 2]
            fx, fy, cx, cy, bf = (self.cam[k][self.ek] for k in ("fx", "fy", "cx", "cy", "mbf"))
            invz = (1.0 / z).astype(F32).astype(F64)            # cam_project's `const float invz` (types_six_dof_expmap.cpp:191)
            p0 = (x * invz) * fx + cx
            s0, s1, s2 = self.ox - p0, self.oy - ((y * invz) * fy + cy), self.ur - (p0 - bf * invz)
            m0, m1 = self.ox - ((fx * x) / z + cx), self.oy - ((fy * y) / z + cy)     # Pinhole::project
            st = self.stereo
            e = np.stack([np.where(st, s0, m0), np.where(st, s1, m1), np.where(st, s2, 0.0)], -1)
            w = self.w
            chi2 = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
            chi2 = np.where(st, chi2 + e[:, 2] * (w * e[:, 2]), chi2)
        return e, p, chi2

    def huber(self, chi2):
        """RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91)"""
        with np.errstate(all="ignore"):
            dsqr = self.delta * self.delta
            inl = chi2 <= dsqr
            s = np.sqrt(chi2)
            return np.where(inl, chi2, (2 * s) * self.delta - dsqr), np.where(inl, 1.0, self.delta / s)

    def jacobians(self, q, p):
        """-> Ja [E, 3, 3] (_jacobianOplusXi: the point), Jb [E, 3, 6] (_jacobianOplusXj: the pose)"""
        with np.errstate(all="ignore"):
            qe = q[self.ek]
            qx, qy, qz, qw = qe[:, 0], qe[:, 1], qe[:, 2], qe[:, 3]
            tx, ty, tz = 2 * qx, 2 * qy, 2 * qz                 # Eigen's toRotationMatrix
            twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * qw, ty * qw, tz * qw, tx * qx, ty * qx, tz * qx, ty * qy, tz * qy, tz * qz
            R = [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]
            x, y, z = p[:, 0], p[:, 1], p[:, 2]
            fx, fy, bf = (self.cam[k][self.ek] for k in ("fx", "fy", "mbf"))
            z_2 = z * z
            E = self.E
            Sa, Sb = np.zeros((E, 3, 3), F64), np.zeros((E, 3, 6), F64)       # types_six_dof_expmap.cpp:228-274
            for j in range(3):
                Sa[:, 0, j] = (-fx * R[0][j]) / z + ((fx * x) * R[2][j]) / z_2
                Sa[:, 1, j] = (-fy * R[1][j]) / z + ((fy * y) * R[2][j]) / z_2
                Sa[:, 2, j] = Sa[:, 0, j] - (bf * R[2][j]) / z_2
            Sb[:, 0, 0] = ((x * y) / z_2) * fx
            Sb[:, 0, 1] = -(1 + ((x * x) / z_2)) * fx
            Sb[:, 0, 2] = (y / z) * fx
            Sb[:, 0, 3] = (-1. / z) * fx
            Sb[:, 0, 5] = (x / z_2) * fx
            Sb[:, 1, 0] = (1 + (y * y) / z_2) * fy
            Sb[:, 1, 1] = ((-x * y) / z_2) * fy
            Sb[:, 1, 2] = (-x / z) * fy
            Sb[:, 1, 4] = (-1. / z) * fy
            Sb[:, 1, 5] = (y / z_2) * fy
            Sb[:, 2, 0] = Sb[:, 0, 0] - (bf * y) / z_2
            Sb[:, 2, 1] = Sb[:, 0, 1] + (bf * x) / z_2
            Sb[:, 2, 2] = Sb[:, 0, 2]
            Sb[:, 2, 3] = Sb[:, 0, 3]
            Sb[:, 2, 5] = Sb[:, 0, 5] - bf / z_2
            a, g, b, d = fx / z, (-fx * x) / (z * z), fy / z, (-fy * y) / (z * z)      # OptimizableTypes.cpp:139-160
            Ma, Mb = np.zeros((E, 3, 3), F64), np.zeros((E, 3, 6), F64)
            for j in range(3):
                Ma[:, 0, j] = (-a) * R[0][j] + (-g) * R[2][j]
                Ma[:, 1, j] = (-b) * R[1][j] + (-d) * R[2][j]
            Mb[:, 0, 0] = -(g * y)
            Mb[:, 0, 1] = -(a * z + g * -x)
            Mb[:, 0, 2] = -(a * -y)
            Mb[:, 0, 3] = -a
            Mb[:, 0, 5] = -g
            Mb[:, 1, 0] = -(b * -z + d * y)
            Mb[:, 1, 1] = -(d * -x)
            Mb[:, 1, 2] = -(b * x)
            Mb[:, 1, 4] = -b
            Mb[:, 1, 5] = -d
            st = self.stereo[:, None, None]
        return np.where(st, Sa, Ma), np.where(st, Sb, Mb)

    def quadratic_forms(self, e, rho1, Ja, Jb):
        """constructQuadraticForm (base_binary_edge.hpp:91-113) per edge -> Hll [E, 6] (upper), bl [E, 3], Hpp [E, 21], bp [E, 6],
        W [E, 6, 3] (Hpl: pose rows, point columns)"""
        st = self.stereo
        with np.errstate(all="ignore"):
            w = self.w
            wr = rho1 * w                                          # robustInformation (base_edge.h:96-100)
            omr = (-(w[:, None] * e)) * rho1[:, None]              # omega_r = -Omega e, times rho'

            def quad(ua, ub):                                      # ua, ub [E, 3]
                t = (ua[:, 0] * wr) * ub[:, 0] + (ua[:, 1] * wr) * ub[:, 1]
                return np.where(st, t + (ua[:, 2] * wr) * ub[:, 2], t)

            def dotr(ua):
                t = ua[:, 0] * omr[:, 0] + ua[:, 1] * omr[:, 1]
                return np.where(st, t + ua[:, 2] * omr[:, 2], t)

            Hll = np.stack([quad(Ja[:, :, a], Ja[:, :, b]) for a in range(3) for b in range(a, 3)], -1)
            bl = np.stack([dotr(Ja[:, :, a]) for a in range(3)], -1)
            Hpp = np.stack([quad(Jb[:, :, a], Jb[:, :, b]) for a in range(6) for b in range(a, 6)], -1)
            bp = np.stack([dotr(Jb[:, :, a]) for a in range(6)], -1)
            W = np.stack([np.stack([quad(Jb[:, :, a], Ja[:, :, b]) for b in range(3)], -1) for a in range(6)], 1)
        return Hll, bl, Hpp, bp, W


UP3 = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
SYM3 = [[0, 1, 2], [1, 3, 4], [2, 4, 5]]
UP6 = [(a, b) for a in range(6) for b in range(a, 6)]


def point_inverse(Hll, bl, lam):
    """[P, 6] upper, [P, 3] -> Dinv [P, 6] upper, db [P, 3] (block_solver.hpp:389-395)"""
    with np.errstate(all="ignore"):
        m00, m01, m02, m11, m12, m22 = Hll[:, 0] + lam, Hll[:, 1], Hll[:, 2], Hll[:, 3] + lam, Hll[:, 4], Hll[:, 5] + lam
        c00, c10, c20 = m11 * m22 - m12 * m12, m12 * m02 - m22 * m01, m01 * m12 - m02 * m11
        det = (c00 * m00 + c10 * m01) + c20 * m02
        inv = 1.0 / det
        D = np.stack([c00 * inv, c10 * inv, c20 * inv, (m22 * m00 - m02 * m02) * inv, (m02 * m01 - m00 * m12) * inv,
                      (m00 * m11 - m01 * m01) * inv], -1)
        db = sym3_times(D, bl)
    return D, db


def sym3_times(D, v):
    with np.errstate(all="ignore"):
        return np.stack([(D[:, SYM3[r][0]] * v[:, 0] + D[:, SYM3[r][1]] * v[:, 1]) + D[:, SYM3[r][2]] * v[:, 2] for r in range(3)], -1)


def ldlt_solve(A, b, x):
    """L D L^T of the symmetric A (its lower triangle is read; A is overwritten), right-looking: column m takes l_im (l_km d_m) off
    entry (i, k) for m ascending.  Rows whose l is exactly zero are skipped (they would subtract nothing).  Then L y = b and
    D L^T x = y column by column.  -> ok; x is replaced only when ok"""
    n = len(b)
    rd = np.zeros(n, F64)
    with np.errstate(all="ignore"):
        for j in range(n):
            d = A[j, j]
            if not d > 0:
                return False
            r = 1.0 / d
            rd[j] = r
            nz = j + 1 + np.nonzero(A[j + 1:, j])[0]
            if len(nz):
                v = A[nz, j].copy()
                l = v * r
                A[nz, j] = l
                A[np.ix_(nz, nz)] -= l[:, None] * v[None, :]
        y = np.array(b, F64)
        for m in range(n):
            nz = m + 1 + np.nonzero(A[m + 1:, m])[0]
            if len(nz):
                y[nz] -= A[nz, m] * y[m]
        y *= rd
        for m in range(n - 1, -1, -1):
            nz = np.nonzero(A[m, :m])[0]
            if len(nz):
                y[nz] -= A[m, nz] * y[m]
    x[:] = y
    return True


# ------------------------------------------------------------------------------------------------------------ the routine
def levenberg(pr, q, t, X, variant, iterations, huber, stop=False, solve=ldlt_solve):
    """g2o's loop (sparse_optimizer.cpp:376-389 around OptimizationAlgorithmLevenberg::solve, levenberg.cpp:61-170) from the state
    q [K, 4], t [K, 3], X [P, 3] of the Problem pr; q and t are updated in place.  huber: chi2 -> (rho, rho'); stop: terminate()
    holds; solve: the solver of the reduced system.
    -> q, t, X, lambda, dict(iterations, trials, rejected_trials, chi2_initial, chi2_final)"""
    order = _order(variant)
    pl = pr.plan
    P, E, Kf = pr.P, pr.E, pl.Kf
    res = dict(iterations=0, trials=0, rejected_trials=0, chi2_initial=0.0, chi2_final=0.0)
    n = 6 * Kf
    x = np.zeros(n + 3 * P, F64)
    lam, ni, n_bad, ok = 0.0, 2.0, 0, E > 0
    it = 0
    while it < iterations and ok and not stop:                   # sparse_optimizer.cpp:376 (terminate())
        # ---- OptimizationAlgorithmLevenberg::solve ----
        e, p, chi2 = pr.error(q, t, X)                           # :75
        rho0, rho1 = huber(chi2)
        current = float(ordered_sum(rho0[:, None], order)[0])    # :82
        ini = current
        Ja, Jb = pr.jacobians(q, p)                              # :87 buildSystem
        eHll, ebl, eHpp, ebp, W = pr.quadratic_forms(e, rho1, Ja, Jb)
        Hl = seg_sum(np.concatenate([eHll, ebl], 1), pr.ep, P, order)
        Hll, bl = Hl[:, :6], Hl[:, 6:]
        Hp = seg_sum(np.concatenate([eHpp, ebp], 1)[pl.kf_edge], pl.kf_seg, Kf, order)
        Hpp, bp = Hp[:, :21], Hp[:, 21:]
        if it == 0:                                              # :93-97, computeLambdaInit :172-186 (every non-fixed vertex)
            res["chi2_initial"] = current
            diag = np.concatenate([np.abs(Hpp[:, [0, 6, 11, 15, 18, 20]]).ravel(), np.abs(Hll[:, [0, 3, 5]]).ravel()])
            lam, ni, n_bad = 1e-5 * float(max(diag.max() if len(diag) else 0.0, 0.0)), 2.0, 0
        rho, qmax = 0.0, 0
        while True:
            bq, bt, bX = q.copy(), t.copy(), X.copy()            # push (:103)
            if variant == "dense":
                ok2 = _solve_dense(pr, Hpp, bp, Hll, bl, W, lam, x)
            else:
                ok2 = _solve_schur(pr, Hpp, bp, Hll, bl, W, lam, x, order, solve)
            for i in range(Kf):                                  # update (:115): VertexSE3Expmap::oplusImpl
                k = pl.kf_of_free[i]
                nq, nt = oplus(list(q[k]), list(t[k]), [float(v) for v in x[6 * i:6 * i + 6]])
                q[k], t[k] = nq, nt
            X = X + x[n:].reshape(P, 3)                          # VertexSBAPointXYZ::oplusImpl
            _, _, chi2 = pr.error(q, t, X)                       # :123
            r0, _ = huber(chi2)
            temp = float(ordered_sum(r0[:, None], order)[0])     # :124
            if not ok2:
                temp = DBL_MAX                                   # :126-127
            b_all = np.concatenate([bp.ravel(), bl.ravel()])
            with np.errstate(all="ignore"):
                scale = float(ordered_sum((x * (lam * x + b_all))[:, None], order)[0]) + 1e-3   # computeScale :188-195, :131
                rho = float((F64(current) - F64(temp)) / F64(scale))
            res["trials"] += 1
            if rho > 0 and math.isfinite(temp):                  # :134-142
                yy = 2 * rho - 1
                alpha = min(1. - (yy * yy) * yy, 2. / 3.)
                lam *= max(1. / 3., alpha)
                ni = 2.0
                current = temp
            else:                                                # :143-147
                lam *= ni
                ni *= 2
                q, t, X = bq, bt, bX
                res["rejected_trials"] += 1
            qmax += 1
            if not (rho < 0 and qmax < 10):                      # :149
                break
        res["iterations"] += 1
        res["chi2_final"] = current
        it += 1
        if qmax == 10 or rho == 0:                               # :151-155
            ok = False
            continue
        if (ini - current) * 1e3 < ini:                          # :157-162
            n_bad += 1
        else:
            n_bad = 0
        if n_bad >= 3:                                           # :164-167
            ok = False
    if res["iterations"] == 0:
        res["chi2_final"] = res["chi2_initial"]
    return q, t, X, lam, res


def local_ba(s, variant="forward", max_iterations=10):
    """s: a scene of make_scene (or any dict with kf, pos_w, edge_kf, edge_point, xy, u_right, inv_sigma2).
    -> dict(status, iterations, trials, rejected_trials, n_outliers, kf_qt_d [K, 7], kf_qt (float32), pos_d, pos, outlier [E],
    chi2 [E] (at the final estimate), depth [E], chi2_initial, chi2_final, lambda_final)"""
    pr = Problem(s)
    K, E, Kf = pr.K, pr.E, pr.plan.Kf
    kf = s["kf"]
    q_in, t_in, X_in = np.asarray(kf["q"]), np.asarray(kf["t"]), np.asarray(s["pos_w"])
    res = dict(status=0, iterations=0, trials=0, rejected_trials=0, n_outliers=0, chi2_initial=0.0, chi2_final=0.0, lambda_final=0.0)

    def untouched(status):
        res.update(status=status, kf_qt_d=np.concatenate([q_in, t_in], 1).astype(F64), pos_d=X_in.astype(F64),
                   outlier=np.zeros(E, bool), chi2=np.zeros(E), depth=np.zeros(E))
        res["kf_qt"], res["pos"] = res["kf_qt_d"].astype(F32), res["pos_d"].astype(F32)
        return res

    if Kf == K:                                                  # :1098-1102
        return untouched(1)
    q = np.array([normalize_rotation(v) for v in q_in.astype(F64)])      # :1134, :1150 (SE3Quat's constructor normalises)
    t = t_in.astype(F64).copy()
    X = X_in.astype(F64).copy()                                  # :1200
    q, t, X, lam, counts_ = levenberg(pr, q, t, X, variant, max_iterations, pr.huber)
    res.update(counts_)
    # ---- :1331-1373 ----
    _, p, chi2 = pr.error(q, t, X)
    with np.errstate(all="ignore"):
        f = chi2.astype(F32).astype(F64)
        outlier = (f > np.where(pr.stereo, CHI2_STEREO, CHI2_MONO)) | ~(p[:, 2] > 0.0)
    qt = np.concatenate([q, t], 1)
    qt[pr.fixed] = np.concatenate([q_in, t_in], 1).astype(F64)[pr.fixed]     # a fixed KeyFrame's output repeats its input
    res.update(kf_qt_d=qt, pos_d=X, outlier=outlier, n_outliers=int(outlier.sum()), chi2=chi2, depth=p[:, 2], lambda_final=lam)
    res["kf_qt"], res["pos"] = qt.astype(F32), X.astype(F32)     # :1393, :1402
    return res


def _point_update(pr, W, bl, Dinv, x, order):
    """block_solver.hpp:461-481: xl = Dinv (bl - sum_e W_e^T xp)"""
    pl = pr.plan
    P, n = pr.P, 6 * pl.Kf
    fe = np.nonzero(pl.edge_free >= 0)[0]
    with np.errstate(all="ignore"):
        xp = x[:n].reshape(-1, 6)[pl.edge_free[fe]] if len(fe) else np.zeros((0, 6))
        tt = np.zeros((len(fe), 3), F64)
        for r in range(6):                                       # rightMultiply: cl += W^T (-xp), r ascending
            tt = tt + W[fe, r, :] * (-xp[:, r])[:, None]
    seg = np.concatenate([np.arange(P), pr.ep[fe]])
    terms = np.concatenate([bl, tt])
    o = np.argsort(seg, kind="stable")                           # bl first, then the point's edges in order
    cl = seg_sum(terms[o], seg[o], P, order)
    return sym3_times(Dinv, cl)


def _solve_schur(pr, Hpp, bp, Hll, bl, W, lam, x, order, solve=ldlt_solve):
    pl = pr.plan
    Kf, P, n = pl.Kf, pr.P, 6 * pl.Kf
    Dinv, db = point_inverse(Hll, bl, lam)
    xs = x[:n].copy()
    ok = True
    if Kf:
        with np.errstate(all="ignore"):
            a, b = pl.pair_a, pl.pair_b
            Di = Dinv[pr.ep[a]]
            Wa, Wb = W[a], W[b]
            Y = np.stack([(Wa[:, :, 0] * Di[:, SYM3[c][0], None] + Wa[:, :, 1] * Di[:, SYM3[c][1], None]) + Wa[:, :, 2] * Di[:, SYM3[c][2], None]
                          for c in range(3)], -1)                # BDinv = Bi Dinv [m, 6, 3]
            T = (Y[:, :, None, 0] * Wb[:, None, :, 0] + Y[:, :, None, 1] * Wb[:, None, :, 1]) + Y[:, :, None, 2] * Wb[:, None, :, 2]   # BDinv Bj^T
            Hd = np.zeros((Kf, 6, 6), F64)                       # Hpp + lambda I (setLambda), full from the upper triangle
            for k, (r, c) in enumerate(UP6):
                Hd[:, r, c] = Hd[:, c, r] = Hpp[:, k]
            Hd[:, range(6), range(6)] += lam
            seg = np.concatenate([pl.diag_pair, pl.pair_seg])    # Hschur = Hpp, then -= every term in landmark order (:374, :429)
            terms = np.concatenate([Hd.reshape(Kf, 36), -T.reshape(-1, 36)])
            o = np.argsort(seg, kind="stable")
            blocks = seg_sum(terms[o], seg[o], len(pl.pair_key), order).reshape(-1, 6, 6)
            S = np.zeros((n, n), F64)
            for k in range(len(pl.pair_key)):
                i, j = int(pl.pair_i[k]), int(pl.pair_j[k])
                if i == j:
                    S[6 * i:6 * i + 6, 6 * i:6 * i + 6] = np.triu(blocks[k]).T + np.triu(blocks[k], 1)   # the upper triangle's values
                else:
                    S[6 * j:6 * j + 6, 6 * i:6 * i + 6] = blocks[k].T
            fe = pl.kf_edge
            dbe = db[pr.ep[fe]]
            ct = np.stack([(W[fe, r, 0] * dbe[:, 0] + W[fe, r, 1] * dbe[:, 1]) + W[fe, r, 2] * dbe[:, 2] for r in range(6)], -1)   # Bi db (:413)
            coeff = seg_sum(ct, pl.kf_seg, Kf, order)
            bs = (bp - coeff).ravel()                            # :436-439
        ok = solve(S, bs, xs)
        if not ok:
            return False                                         # :456-457: x as it was
    x[:n] = xs
    x[n:] = _point_update(pr, W, bl, Dinv, x, order).ravel()
    return True


def _solve_dense(pr, Hpp, bp, Hll, bl, W, lam, x):
    """the full system, the points first: [[Hll + lambda I, W^T], [W, Hpp + lambda I]] [xl; xp] = [bl; bp]"""
    pl = pr.plan
    Kf, P, n = pl.Kf, pr.P, 6 * pl.Kf
    N = 3 * P + n
    A = np.zeros((N, N), F64)
    for k, (r, c) in enumerate(UP3):
        A[3 * np.arange(P) + c, 3 * np.arange(P) + r] = Hll[:, k] + (lam if r == c else 0.0)
    for k, (r, c) in enumerate(UP6):
        A[3 * P + 6 * np.arange(Kf) + c, 3 * P + 6 * np.arange(Kf) + r] = Hpp[:, k] + (lam if r == c else 0.0)
    fe = np.nonzero(pl.edge_free >= 0)[0]
    for r in range(6):
        for c in range(3):
            np.add.at(A, (3 * P + 6 * pl.edge_free[fe] + r, 3 * pr.ep[fe] + c), W[fe, r, c])
    sol = np.zeros(N, F64)
    if not ldlt_solve(A, np.concatenate([bl.ravel(), bp.ravel()]), sol):
        return False
    x[:n], x[n:] = sol[3 * P:], sol[:3 * P]
    return True


# ---------------------------------------------------------------------------------------------------------------- scenes
KF_DTYPE = np.dtype([("q", "<f4", 4), ("t", "<f4", 3), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("mbf", "<f4"),
                     ("fixed", "<i4")])      # msorb_ba_keyframe


def make_scene(seed, free, fixed, points, stereo=0.6, degree=4, outliers=0.0, noise=1.0, rot_deg=1.0, trans=0.1, point_err=0.03,
               init_fixed=0, single_obs=(0, 0), fixed_only=0, see_all=0, edges=None, behind=False, max_iterations=10, dtype=F32):
    """free + fixed KeyFrames around a KITTI-like camera and `points` points in front of them.  The KeyFrames come local first
    (free, of which the first `init_fixed` carry fixed = 1: the InitKFid KeyFrame, :1136), then the fixed cameras.  Every point is
    seen by `degree` KeyFrames on average (at least 2, one of them free unless told otherwise); stereo: share of stereo edges.
    single_obs = (s, m): s stereo and m mono points with ONE edge; fixed_only: points seen by fixed KeyFrames only; see_all: points
    seen by every KeyFrame; edges: trim or extend to exactly this many edges; behind: the last fixed KeyFrame faces away and sees
    one point (at an unrelated pixel; "exact": at the pinhole image of the point, so the edge has no error and a negative depth).  noise in px at level 0; rot_deg / trans: the free KeyFrames' initial error; point_err: the points' initial error as
    a share of their depth; outliers: share of edges with a gross error of 20-200 px.
    -> dict(kf (KF_DTYPE, or a dict of float64 arrays with dtype=float64), pos_w, edge_kf, edge_point, xy, u_right, inv_sigma2,
    q_true, t_true, X_true, planted [E], median_depth, max_iterations)"""
    rng = np.random.default_rng(seed)
    cam = {k: float(F32(v)) for k, v in pc.KITTI.items()}
    K = free + fixed
    n_fixed_total = fixed + init_fixed
    # true poses: the base camera moved by up to 2 m sideways / forward and turned by up to 8 degrees
    q_true = np.array([pc._quat_from_axis_angle(rng.normal(size=3), math.radians(rng.uniform(0, 8))) for _ in range(K)])
    t_true = rng.uniform(-1, 1, (K, 3)) * np.array([2.0, 0.5, 2.0])
    if behind:
        q_true[K - 1] = pc._quat_mul(pc._quat_from_axis_angle([0, 1, 0], math.pi), q_true[K - 1])
    u, v, z = rng.uniform(130, 1200, points), rng.uniform(5, 370, points), rng.uniform(6, 40, points)
    X_true = np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], -1)     # the base camera = the world
    is_fixed = np.zeros(K, bool)
    is_fixed[free:] = True
    is_fixed[:init_fixed] = True
    usable = np.arange(K - 1 if behind else K)
    ek, ep = [], []
    for p in range(points):
        if p < see_all:
            ks = usable.copy()
        elif p < see_all + single_obs[0] + single_obs[1]:
            ks = rng.choice(np.nonzero(~is_fixed)[0], 1)
        elif p < see_all + sum(single_obs) + fixed_only:
            ks = rng.choice(np.nonzero(is_fixed[:len(usable)])[0], min(2, int(is_fixed[:len(usable)].sum())), replace=False)
        else:
            d = int(np.clip(rng.poisson(degree), 2, len(usable)))
            ks = rng.choice(usable, d, replace=False)
            if is_fixed[ks].all() and (~is_fixed).any():
                ks[0] = rng.choice(np.nonzero(~is_fixed)[0])
        ks = rng.permutation(ks)        # the reference walks a map keyed by pointer: any order
        ek += list(ks)
        ep += [p] * len(ks)
    if behind:
        ek.append(K - 1)
        ep.append(points - 1)
    ek, ep = np.array(ek, np.int32), np.array(ep, np.int32)
    if edges is not None:
        while len(ek) > edges:          # drop edges of the best-observed points, from the back
            cnt = np.bincount(ep, minlength=points)
            e = max(np.nonzero(cnt[ep] == cnt.max())[0])
            ek, ep = np.delete(ek, e), np.delete(ep, e)
        while len(ek) < edges:          # add an edge to a point that a KeyFrame does not see yet
            p = int(rng.integers(see_all + sum(single_obs) + fixed_only, points))
            rest = np.setdiff1d(usable, ek[ep == p])
            if len(rest):
                at = int(np.searchsorted(ep, p, side="right"))
                ek, ep = np.insert(ek, at, rng.choice(rest)), np.insert(ep, at, p)
    E = len(ek)
    Xc = rotate((q_true[ek, 0], q_true[ek, 1], q_true[ek, 2], q_true[ek, 3]), X_true[ep]) + t_true[ek]
    pu, pv = cam["fx"] * Xc[:, 0] / Xc[:, 2] + cam["cx"], cam["fy"] * Xc[:, 1] / Xc[:, 2] + cam["cy"]
    levels = rng.integers(0, 8, E)
    sigma = 1.2 ** levels
    inv_sigma2 = (1.0 / (sigma * sigma)).astype(F32)
    is_stereo = rng.uniform(size=E) < stereo
    single = np.arange(points) < see_all + sum(single_obs)
    first_single = see_all
    for p in range(first_single, first_single + sum(single_obs)):
        is_stereo[ep == p] = p < first_single + single_obs[0]
    xy = np.stack([pu, pv], -1) + rng.normal(size=(E, 2)) * (noise * sigma)[:, None]
    ur = pu - cam["mbf"] / Xc[:, 2] + rng.normal(size=E) * noise * sigma
    planted = rng.uniform(size=E) < outliers
    planted &= ~single[ep] | (np.arange(points) < see_all)[ep]
    ang, mag = rng.uniform(0, 2 * math.pi, E), rng.uniform(20, 200, E)
    xy[planted] += (np.stack([np.cos(ang), np.sin(ang)], -1) * mag[:, None])[planted]
    if behind:
        if behind != "exact":           # "exact": the observation is the pinhole image of the point behind the camera: no error, no depth
            xy[-1] = (600.0, 180.0)
        is_stereo[-1] = False
        planted[-1] = True
    ur = np.where(is_stereo, ur, -1.0)
    # the initial estimate
    q0, t0 = q_true.copy(), t_true.copy()
    for k in range(K):
        if not is_fixed[k] and (rot_deg or trans):
            dq = pc._quat_from_axis_angle(rng.normal(size=3), math.radians(rot_deg))
            dt = rng.normal(size=3)
            q0[k] = pc._quat_mul(dq, q_true[k])
            t0[k] = rotate(dq, t_true[k]) + dt / np.linalg.norm(dt) * trans
    q0 /= np.linalg.norm(q0, axis=1)[:, None]
    X0 = X_true + rng.normal(size=(points, 3)) * (point_err * z)[:, None]
    if dtype == F64:
        kf = dict(q=q0, t=t0, fixed=is_fixed.astype(np.int32), **{k: np.full(K, cam[k]) for k in cam})
    else:
        kf = np.zeros(K, KF_DTYPE)
        kf["q"], kf["t"], kf["fixed"] = q0, t0, is_fixed
        for k in cam:
            kf[k] = cam[k]
    assert n_fixed_total == int(is_fixed.sum())
    return dict(kf=kf, pos_w=X0.astype(dtype), edge_kf=ek, edge_point=ep, xy=xy.astype(dtype), u_right=ur.astype(dtype),
                inv_sigma2=inv_sigma2.astype(dtype), q_true=q_true, t_true=t_true, X_true=X_true, planted=planted,
                median_depth=float(np.median(z)), max_iterations=max_iterations, depth=z)


# name -> make_scene arguments.  A scene that misses a condition of tests/test_local_ba_cpu.py is re-seeded HERE; no bound moves.
_OUTLIERS = dict(seed=14, free=8, fixed=4, points=200, outliers=0.2)
SCENES = {
    "k1": dict(seed=1, free=1, fixed=2, points=12, stereo=1.0, degree=3),
    "k2": dict(seed=2, free=2, fixed=1, points=9, degree=3),
    "init_kf": dict(seed=3, free=3, fixed=0, init_fixed=1, points=30, degree=3),
    "no_fixed": dict(seed=4, free=3, fixed=0, points=20, degree=3),
    "mono_only": dict(seed=5, free=4, fixed=3, points=60, stereo=0.0),
    "stereo_only": dict(seed=6, free=4, fixed=2, points=60, stereo=1.0),
    "single_obs": dict(seed=7, free=4, fixed=2, points=40, single_obs=(6, 4)),
    "fixed_only_point": dict(seed=8, free=4, fixed=3, points=40, fixed_only=5),
    "deg_hi": dict(seed=9, free=33, fixed=5, points=80, see_all=1, degree=6),
    "k33": dict(seed=10, free=33, fixed=5, points=300, degree=6),
    "p65": dict(seed=11, free=6, fixed=3, points=65),
    "p257": dict(seed=12, free=6, fixed=3, points=257),
    "e1025": dict(seed=13, free=6, fixed=3, points=250, edges=1025),
    "outliers": _OUTLIERS,
    "rejected_trials": dict(seed=15, free=8, fixed=4, points=200, outliers=0.4, rot_deg=5.0, trans=0.5),
    "behind": dict(seed=16, free=4, fixed=2, points=40, behind=True),
    "it1": dict(_OUTLIERS, max_iterations=1),
    "it3": dict(_OUTLIERS, max_iterations=3),
    "kitti_like": dict(seed=17, free=12, fixed=6, points=600, degree=6, outliers=0.05),
}
STRUCTURAL = ("k1", "k2", "init_kf", "mono_only", "stereo_only", "single_obs", "fixed_only_point", "deg_hi", "k33", "p65", "p257",
              "e1025", "it1", "it3")
OTHERS = ("outliers", "rejected_trials", "behind", "kitti_like")

_scene_cache, _ref_cache = {}, {}


def scene(name):
    if name not in _scene_cache:
        _scene_cache[name] = make_scene(**SCENES[name])
    return _scene_cache[name]


def reference(name, variant="forward"):
    """the restatement's result on a named scene, computed once per process"""
    if (name, variant) not in _ref_cache:
        s = scene(name)
        _ref_cache[name, variant] = local_ba(s, variant, s["max_iterations"])
    return _ref_cache[name, variant]


def thresholds(s):
    return np.where(np.asarray(s["u_right"]) >= 0, CHI2_STEREO, CHI2_MONO)


def counts(r):
    return (r["status"], r["iterations"], r["trials"], r["rejected_trials"])


def variants_agree(name):
    return len({counts(reference(name, v)) for v in VARIANTS}) == 1


def estimate_distance(s, a, b):
    """the largest difference of two results: quaternion components (sign-aligned), translation over the scene's median depth,
    point position over its depth -> (poses, points)"""
    qa, qb = a["kf_qt_d"][:, :4], b["kf_qt_d"][:, :4]
    sign = np.where(np.sum(qa * qb, 1) < 0, -1.0, 1.0)[:, None]
    dq = np.abs(sign * qa - qb).max(initial=0.0)
    dt = np.abs(a["kf_qt_d"][:, 4:] - b["kf_qt_d"][:, 4:]).max(initial=0.0) / s["median_depth"]
    dp = (np.abs(a["pos_d"] - b["pos_d"]) / s["depth"][:, None]).max(initial=0.0)
    return float(max(dq, dt)), float(dp)


def smallest_movement(s, r):
    """how far the free vertex that moved least went from its input, in the units of estimate_distance"""
    kf = s["kf"]
    free = ~np.asarray(kf["fixed"]).astype(bool)
    q0 = np.array([normalize_rotation(v) for v in np.asarray(kf["q"], F64)])
    dq = np.abs(q0 - r["kf_qt_d"][:, :4]).max(1)
    dt = np.abs(np.asarray(kf["t"], F64) - r["kf_qt_d"][:, 4:]).max(1) / s["median_depth"]
    dp = (np.abs(np.asarray(s["pos_w"], F64) - r["pos_d"]) / s["depth"][:, None]).max(1)
    return float(min(np.maximum(dq, dt)[free].min(initial=math.inf), dp.min(initial=math.inf)))


def measure():
    """D: the largest difference between any two variants (estimate_distance); C: the same for an edge's final chi2, relative to
    max(chi2, threshold); margin: the smallest relative distance of any final chi2 from its threshold; per scene and overall"""
    per, D, C, margin = {}, 0.0, 0.0, math.inf
    for name in SCENES:
        s = scene(name)
        refs = [reference(name, v) for v in VARIANTS]
        th = thresholds(s)
        d = c = 0.0
        m = math.inf
        if refs[0]["status"] == 0:
            for r in refs:
                with np.errstate(all="ignore"):
                    m = min(m, float(np.nanmin(np.abs(r["chi2"] - th) / th)))
            for a in range(len(refs)):
                for b in range(a + 1, len(refs)):
                    d = max(d, *estimate_distance(s, refs[a], refs[b]))
                    ca, cb = refs[a]["chi2"], refs[b]["chi2"]
                    with np.errstate(all="ignore"):
                        c = max(c, float(np.nanmax(np.abs(ca - cb) / np.maximum(np.maximum(ca, cb), th))))
        per[name] = dict(D=d, C=c, margin=m if math.isfinite(m) else None, variants_agree=variants_agree(name),
                         movement=smallest_movement(s, refs[0]) if refs[0]["status"] == 0 else None)
        D, C, margin = max(D, d), max(C, c), min(margin, m)
    return dict(D=D, C=C, bound=16 * D, margin=margin, scenes=per)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_ba_sensitivity.json")

if __name__ == "__main__":
    if "--measure" in sys.argv:
        t0 = time.perf_counter()
        m = measure()
        with open(GOLDEN, "w") as f:
            json.dump(m, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps({k: m[k] for k in ("D", "C", "bound", "margin")}), f"{time.perf_counter() - t0:.1f} s")
        for name, v in m["scenes"].items():
            r = reference(name)
            print(f"{name:18s} D={v['D']:.2e} C={v['C']:.2e} margin={v['margin']} move={v['movement']} agree={v['variants_agree']} "
                  f"counts={[counts(reference(name, x)) for x in VARIANTS]} E={len(r['outlier'])} out={r['n_outliers']} "
                  f"chi2 {r['chi2_initial']:.1f}->{r['chi2_final']:.1f}")
    else:
        print(__doc__)
