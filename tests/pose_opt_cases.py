"""Optimizer::PoseOptimization (src/Optimizer.cc:759-1037) restated in float64 numpy, with the g2o pieces it runs
(Thirdparty/g2o/g2o: core/optimization_algorithm_levenberg.cpp:61-195, core/sparse_optimizer.cpp:354-419,
core/base_unary_edge.hpp:43-72, core/base_edge.h:60,96-100, core/robust_kernel_impl.cpp:65-91, types/se3quat.h,
types/types_six_dof_expmap.{h,cpp}, src/OptimizableTypes.cpp:49-63, src/CameraModels/Pinhole.cpp:35-41,71-81), the scene
generator and the scene list of the GPU tests.  No GPU, no library.

`python tests/pose_opt_cases.py --measure` writes tests/golden/pose_opt_sensitivity.json.

What the restatement fixes where the reference leaves it to Eigen / libm (ms-slam_amd/csrc/pose_opt.hip does the same):
  * a product of small matrices is the plain row-by-column sum, left to right, without fused multiply-adds;
  * pow(y, 3) is (y*y)*y;
  * the dense solver is the square-root-free Cholesky L D L^T of H + lambda I without pivoting, one reciprocal per pivot
    (LinearSolverDense uses Eigen's pivoted LDLT; the two agree except in rounding), a pivot that is not positive is its "not
    positive" answer, and x then keeps what it held;
  * `sum_order` fixes how H, b and the cost are added over the active edges: 'forward' (edge 0 first, what g2o does over its
    edge list), 'reverse', 'pairwise' (a balanced tree).
"""
import json
import math
import os
import sys

import numpy as np

F32, F64 = np.float32, np.float64
KITTI = dict(fx=718.856, fy=718.856, cx=607.19, cy=185.22, mbf=386.14)
DELTA_MONO = float(F32(math.sqrt(5.991)))     # Optimizer.cc:796
DELTA_STEREO = float(F32(math.sqrt(7.815)))   # Optimizer.cc:797
CHI2_MONO, CHI2_STEREO = F32(5.991), F32(7.815)   # :941-942
DBL_MAX = sys.float_info.max
ORDERS = ("forward", "reverse", "pairwise")


# ---------------------------------------------------------------------------------------------------------------- sums
def ordered_sum(terms, order):
    """terms [m, k] -> [k], the additions made in the named order (m == 0: zeros)."""
    terms = np.asarray(terms, F64)
    if terms.shape[0] == 0:
        return np.zeros(terms.shape[1], F64)
    if order == "forward":
        return np.cumsum(terms, axis=0)[-1]          # cumsum adds one row after the other
    if order == "reverse":
        return np.cumsum(terms[::-1], axis=0)[-1]
    if order == "pairwise":
        a = terms
        while a.shape[0] > 1:
            if a.shape[0] & 1:
                a = np.concatenate([a, np.zeros((1, a.shape[1]), F64)])
            a = a[0::2] + a[1::2]
        return a[0]
    raise ValueError(order)


# ------------------------------------------------------------------------------------------------------------- SE3Quat
def rotate(q, v):
    """Eigen QuaternionBase::_transformVector: uv = 2 vec x v; v + w uv + vec x uv.  q = (x, y, z, w); v [..., 3]"""
    qx, qy, qz, qw = q
    X, Y, Z = v[..., 0], v[..., 1], v[..., 2]
    ux, uy, uz = qy * Z - qz * Y, qz * X - qx * Z, qx * Y - qy * X
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return np.stack([(X + qw * ux) + (qy * uz - qz * uy), (Y + qw * uy) + (qz * ux - qx * uz), (Z + qw * uz) + (qx * uy - qy * ux)], -1)


def normalize_rotation(q):
    """se3quat.h:280-285"""
    q = [float(c) for c in q]
    if q[3] < 0:
        q = [c * -1 for c in q]
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [c / n for c in q]


def se3_exp(u):
    """SE3Quat::exp (se3quat.h:223-257) -> (q, t); Quaterniond(R) as Eigen converts a rotation matrix"""
    ox, oy, oz = u[0], u[1], u[2]
    theta = math.sqrt((ox * ox + oy * oy) + oz * oz)
    O = [[0.0, -oz, oy], [oz, 0.0, -ox], [-oy, ox, 0.0]]
    O2 = [[(O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j] for j in range(3)] for i in range(3)]
    eye = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    if theta < 0.00001:       # :237-243
        R = [[(eye[i][j] + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
        V = R
    else:                     # :244-255
        s, c = math.sin(theta), math.cos(theta)
        a, b, d = s / theta, (1 - c) / (theta * theta), (theta - s) / ((theta * theta) * theta)
        R = [[(eye[i][j] + a * O[i][j]) + b * O2[i][j] for j in range(3)] for i in range(3)]
        V = [[(eye[i][j] + b * O[i][j]) + d * O2[i][j] for j in range(3)] for i in range(3)]
    q = [0.0] * 4
    t = (R[0][0] + R[1][1]) + R[2][2]
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[2][1] - R[1][2]) * t
        q[1] = (R[0][2] - R[2][0]) * t
        q[2] = (R[1][0] - R[0][1]) * t
    else:
        i = 0
        if R[1][1] > R[0][0]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(((R[i][i] - R[j][j]) - R[k][k]) + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k][j] - R[j][k]) * t
        q[j] = (R[j][i] + R[i][j]) * t
        q[k] = (R[k][i] + R[i][k]) * t
    tr = [(V[i][0] * u[3] + V[i][1] * u[4]) + V[i][2] * u[5] for i in range(3)]
    return normalize_rotation(q), tr      # SE3Quat(q, t): :62-64


def oplus(q, t, x):
    """VertexSE3Expmap::oplusImpl (types_six_dof_expmap.h:73-76): exp(x) * estimate, SE3Quat::operator* (se3quat.h:104-110)"""
    eq, et = se3_exp(x)
    r = rotate(eq, np.array(t, F64))
    nt = [et[i] + float(r[i]) for i in range(3)]
    ex, ey, ez, ew = eq
    tx, ty, tz, tw = q
    nq = [((ew * tx + ex * tw) + ey * tz) - ez * ty,
          ((ew * ty + ey * tw) + ez * tx) - ex * tz,
          ((ew * tz + ez * tw) + ex * ty) - ey * tx,
          ((ew * tw - ex * tx) - ey * ty) - ez * tz]
    return normalize_rotation(nq), nt


# --------------------------------------------------------------------------------------------------------------- edges
class Edges:
    """The edges of :802-934 (pinhole arm) as arrays: obs [n, 3] (u_right < 0: a mono edge), w = invSigma2, Xw [n, 3]"""

    def __init__(self, cam, xy, u_right, inv_sigma2, pos_w):
        self.fx, self.fy, self.cx, self.cy, self.bf = (float(F32(cam[k])) for k in ("fx", "fy", "cx", "cy", "mbf"))   # the frame's floats (:856-860)
        self.x = np.asarray(xy, F64).reshape(-1, 2)[:, 0]
        self.y = np.asarray(xy, F64).reshape(-1, 2)[:, 1]
        self.ur = np.asarray(u_right, F64).reshape(-1)
        self.w = np.asarray(inv_sigma2, F64).reshape(-1)
        self.Xw = np.asarray(pos_w, F64).reshape(-1, 3)
        self.n = len(self.ur)
        self.stereo = self.ur >= 0      # :808
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)

    def error(self, q, t):
        """computeError of both edge types -> e [n, 3], camera-frame point [n, 3], chi2 [n] (base_edge.h:60)"""
        with np.errstate(all="ignore"):
            p = rotate(q, self.Xw) + np.array(t, F64)     # SE3Quat::map (:217-220)
            x, y, z = p[:, 0], p[:, 1], p[:, 2]
            invz = (1.0 / z).astype(F32).astype(F64)      # cam_project's `const float invz` (types_six_dof_expmap.cpp:340)
            p0 = (x * invz) * self.fx + self.cx
            s0 = self.x - p0
            s1 = self.y - ((y * invz) * self.fy + self.cy)
            s2 = self.ur - (p0 - self.bf * invz)
            m0 = self.x - ((self.fx * x) / z + self.cx)   # Pinhole::project (Pinhole.cpp:35-41)
            m1 = self.y - ((self.fy * y) / z + self.cy)
            e = np.stack([np.where(self.stereo, s0, m0), np.where(self.stereo, s1, m1), np.where(self.stereo, s2, 0.0)], -1)
            w = self.w
            chi2 = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
            chi2 = np.where(self.stereo, chi2 + e[:, 2] * (w * e[:, 2]), chi2)
        return e, p, chi2

    def jacobian(self, p):
        """[n, 3, 6]: stereo types_six_dof_expmap.cpp:375-403; mono OptimizableTypes.cpp:49-63 with Pinhole::projectJac"""
        with np.errstate(all="ignore"):
            x, y, z = p[:, 0], p[:, 1], p[:, 2]
            fx, fy, bf = self.fx, self.fy, self.bf
            invz = 1.0 / z
            invz_2 = invz * invz
            zero = np.zeros_like(x)
            S = np.empty((self.n, 3, 6), F64)
            S[:, 0, 0] = ((x * y) * invz_2) * fx
            S[:, 0, 1] = -(1 + ((x * x) * invz_2)) * fx
            S[:, 0, 2] = (y * invz) * fx
            S[:, 0, 3] = -invz * fx
            S[:, 0, 4] = zero
            S[:, 0, 5] = (x * invz_2) * fx
            S[:, 1, 0] = (1 + (y * y) * invz_2) * fy
            S[:, 1, 1] = ((-x * y) * invz_2) * fy
            S[:, 1, 2] = (-x * invz) * fy
            S[:, 1, 3] = zero
            S[:, 1, 4] = -invz * fy
            S[:, 1, 5] = (y * invz_2) * fy
            S[:, 2, 0] = S[:, 0, 0] - (bf * y) * invz_2
            S[:, 2, 1] = S[:, 0, 1] + (bf * x) * invz_2
            S[:, 2, 2] = S[:, 0, 2]
            S[:, 2, 3] = S[:, 0, 3]
            S[:, 2, 4] = zero
            S[:, 2, 5] = S[:, 0, 5] - bf * invz_2
            a, g, b, d = fx / z, (-fx * x) / (z * z), fy / z, (-fy * y) / (z * z)
            M = np.zeros((self.n, 3, 6), F64)
            M[:, 0, 0] = -(g * y)
            M[:, 0, 1] = -(a * z + g * -x)
            M[:, 0, 2] = -(a * -y)
            M[:, 0, 3] = -a
            M[:, 0, 5] = -g
            M[:, 1, 0] = -(b * -z + d * y)
            M[:, 1, 1] = -(d * -x)
            M[:, 1, 2] = -(b * x)
            M[:, 1, 4] = -b
            M[:, 1, 5] = -d
        return np.where(self.stereo[:, None, None], S, M)

    def huber(self, chi2, robust):
        """RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91) -> rho, rho'"""
        if not robust:
            return chi2, np.ones_like(chi2)
        with np.errstate(all="ignore"):
            dsqr = self.delta * self.delta                 # setDelta (:65-69)
            inl = chi2 <= dsqr
            s = np.sqrt(chi2)
            rho0 = np.where(inl, chi2, (2 * s) * self.delta - dsqr)
            rho1 = np.where(inl, 1.0, self.delta / s)
        return rho0, rho1


def solve6(Hu, lam, b, x):
    """L D L^T (square-root-free Cholesky, no pivoting, one reciprocal per pivot) of H + lambda I (Hu: the upper triangle, row
    major) and the substitutions -> ok; x is updated in place when ok"""
    L = [[0.0] * 6 for _ in range(6)]
    r = [0.0] * 6
    k = 0
    for i in range(6):
        for j in range(i, 6):
            L[j][i] = float(Hu[k])
            k += 1
            if i == j:
                L[i][i] += lam
    for j in range(6):
        v = [0.0] * 6
        d = L[j][j]
        for m in range(j):
            v[m] = L[j][m] * L[m][m]
            d -= L[j][m] * v[m]
        if not d > 0:
            return False
        L[j][j] = d
        r[j] = 1.0 / d
        for i in range(j + 1, 6):
            s = L[i][j]
            for m in range(j):
                s -= L[i][m] * v[m]
            L[i][j] = s * r[j]
    y = [0.0] * 6
    for i in range(6):
        s = float(b[i])
        for m in range(i):
            s -= L[i][m] * y[m]
        y[i] = s
    for i in range(5, -1, -1):
        s = y[i] * r[i]
        for m in range(i + 1, 6):
            s -= L[m][i] * x[m]
        x[i] = s
    return True


def pose_optimization(cam, q, t, xy, u_right, inv_sigma2, pos_w, sum_order="forward"):
    """-> dict(q, t float32 (what SetPose receives), qd, td, outlier [n] bool, n_initial, n_bad, iterations[4],
    rejected_trials[4], chi2 (per classification: the per-edge doubles that were narrowed and compared))"""
    E = Edges(cam, xy, u_right, inv_sigma2, pos_w)
    n = E.n
    res = dict(n_initial=n, iterations=[-1] * 4, rejected_trials=[-1] * 4, chi2=[], outlier=np.zeros(n, bool))
    qf, tf = np.asarray(q, F32), np.asarray(t, F32)
    if n < 3:                                              # :936-937
        res.update(q=qf.copy(), t=tf.copy(), qd=qf.astype(F64), td=tf.astype(F64), n_bad=n)
        return res
    q0, t0 = normalize_rotation(qf.astype(F64)), [float(v) for v in tf.astype(F64)]   # :774-775
    level = np.zeros(n, bool)           # e->setLevel(1): an outlier
    chi2_state = np.zeros(n, F64)       # chi2() of every edge as the last computeActiveErrors / computeError left it
    th = np.where(E.stereo, CHI2_STEREO, CHI2_MONO).astype(F32)
    x = [0.0] * 6
    n_bad = 0
    for it in range(4):                 # :946
        robust = it < 3                 # :974-975
        cq, ct = list(q0), list(t0)     # :947-948
        n_solve = n_rejected = 0
        act = ~level
        if act.any():                   # sparse_optimizer.cpp:356-359
            lam, ni, n_bad_steps, ok = 0.0, 2.0, 0, True
            i = 0
            while i < 10 and ok:        # sparse_optimizer.cpp:376
                # ---- OptimizationAlgorithmLevenberg::solve ----
                e, p, chi2 = E.error(cq, ct)                       # :75
                chi2_state[act] = chi2[act]
                rho0, rho1 = E.huber(chi2, robust)
                J = E.jacobian(p)                                  # :87 buildSystem
                w = E.w
                wr = rho1 * w                                      # robustInformation (base_edge.h:96-100)
                terms = np.empty((n, 28), F64)
                k = 0
                with np.errstate(all="ignore"):
                    for a in range(6):
                        for c in range(a, 6):                      # base_unary_edge.hpp:63
                            tt = (J[:, 0, a] * wr) * J[:, 0, c] + (J[:, 1, a] * wr) * J[:, 1, c]
                            terms[:, k] = np.where(E.stereo, tt + (J[:, 2, a] * wr) * J[:, 2, c], tt)
                            k += 1
                        tt = ((rho1 * J[:, 0, a]) * w) * e[:, 0] + ((rho1 * J[:, 1, a]) * w) * e[:, 1]   # :62
                        terms[:, 21 + a] = -np.where(E.stereo, tt + ((rho1 * J[:, 2, a]) * w) * e[:, 2], tt)
                    terms[:, 27] = rho0                            # activeRobustChi2 (:82)
                S = ordered_sum(terms[act], sum_order)
                Hu, b = S[:21], S[21:27]
                current = float(S[27])
                ini = current
                if i == 0:                                         # :93-97, computeLambdaInit :172-186
                    max_diag, kk = 0.0, 0
                    for j in range(6):
                        max_diag = max(abs(float(Hu[kk])), max_diag)
                        kk += 6 - j
                    lam, ni, n_bad_steps = 1e-5 * max_diag, 2.0, 0
                rho, qmax = 0.0, 0
                while True:
                    bq, bt = list(cq), list(ct)                    # push (:103)
                    ok2 = solve6(Hu, lam, b, x)                    # :109-110
                    cq, ct = oplus(cq, ct, x)                      # :115
                    e2, _, chi2 = E.error(cq, ct)                  # :123
                    chi2_state[act] = chi2[act]
                    r0, _ = E.huber(chi2, robust)
                    temp = float(ordered_sum(r0[act][:, None], sum_order)[0])   # :124
                    if not ok2:
                        temp = DBL_MAX                             # :126-127
                    with np.errstate(all="ignore"):
                        rho = F64(current) - F64(temp)
                        scale = 0.0                                # computeScale (:188-195)
                        for j in range(6):
                            scale += x[j] * (lam * x[j] + float(b[j]))
                        scale += 1e-3
                        rho = float(rho / F64(scale))
                    if rho > 0 and math.isfinite(temp):            # :134-142
                        yy = 2 * rho - 1
                        alpha = 1. - (yy * yy) * yy
                        alpha = min(alpha, 2. / 3.)
                        lam *= max(1. / 3., alpha)
                        ni = 2.0
                        current = temp
                    else:                                          # :143-147
                        lam *= ni
                        ni *= 2
                        cq, ct = bq, bt
                        n_rejected += 1
                    qmax += 1
                    if not (rho < 0 and qmax < 10):                # :149
                        break
                n_solve += 1
                i += 1
                if qmax == 10 or rho == 0:                         # :151-155
                    ok = False
                    continue
                if (ini - current) * 1e3 < ini:                    # :157-162
                    n_bad_steps += 1
                else:
                    n_bad_steps = 0
                if n_bad_steps >= 3:                               # :164-167
                    ok = False
        res["iterations"][it], res["rejected_trials"][it] = n_solve, n_rejected
        # ---- classification (Optimizer.cc:953-1024) ----
        _, _, fresh = E.error(cq, ct)
        chi2_state[level] = fresh[level]                           # :959-961: only the current outliers are recomputed
        res["chi2"].append(chi2_state.copy())
        with np.errstate(all="ignore"):
            level = chi2_state.astype(F32) > th                    # :963-972 (NaN > th is false)
        n_bad = int(level.sum())
        if n < 10:                                                 # :1026-1027
            break
    res.update(qd=np.array(cq, F64), td=np.array(ct, F64), n_bad=n_bad, outlier=level.copy())
    res["q"], res["t"] = res["qd"].astype(F32), res["td"].astype(F32)   # :1033-1034
    return res


# ------------------------------------------------------------------------------------------------------------ scenes
def _quat_from_axis_angle(axis, angle):
    axis = np.asarray(axis, F64) / np.linalg.norm(axis)
    return np.concatenate([axis * math.sin(angle / 2), [math.cos(angle / 2)]])


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def make_scene(seed, n, stereo=1.0, outliers=0.0, noise=1.0, rot_deg=1.0, trans=0.1, behind=False, garbage=False, dtype=F32):
    """A random pose and n points in front of a KITTI-like camera.  stereo: share of stereo observations; outliers: share with a
    gross error of 20-200 px; noise: sigma in px at level 0 (times the level's scale); rot_deg / trans: the initial pose's error;
    behind: the last point lies behind the camera at the initial pose; garbage: every observation is unrelated to its point.
    -> dict(cam, q, t (initial), xy, u_right, inv_sigma2, pos_w, q_true, t_true, planted [n] bool, median_depth)"""
    rng = np.random.default_rng(seed)
    cam = {k: float(F32(v)) for k, v in KITTI.items()}      # the camera as the frame holds it
    q_true = _quat_from_axis_angle(rng.normal(size=3), math.radians(rng.uniform(0, 30)))
    t_true = rng.uniform(-2, 2, 3)
    u = rng.uniform(130, 1200, n)
    v = rng.uniform(5, 370, n)
    z = rng.uniform(4, 40, n)
    Xc = np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], -1)
    q_inv = q_true * np.array([-1, -1, -1, 1.0])
    Xw = rotate(q_inv, Xc - t_true) if n else np.zeros((0, 3))
    levels = rng.integers(0, 8, n)
    sigma = 1.2 ** levels
    inv_sigma2 = (1.0 / (sigma * sigma)).astype(F32)
    is_stereo = rng.uniform(size=n) < stereo
    ur = u - cam["mbf"] / z
    xy = np.stack([u, v], -1) + rng.normal(size=(n, 2)) * (noise * sigma)[:, None]
    ur = ur + rng.normal(size=n) * noise * sigma
    planted = rng.uniform(size=n) < outliers
    ang = rng.uniform(0, 2 * math.pi, n)
    mag = rng.uniform(20, 200, n)
    xy[planted] += (np.stack([np.cos(ang), np.sin(ang)], -1) * mag[:, None])[planted]
    if garbage:
        xy = np.stack([rng.uniform(0, 1241, n), rng.uniform(0, 376, n)], -1)
        ur = xy[:, 0] - rng.uniform(5, 90, n)
        planted[:] = True
    ur = np.where(is_stereo, np.maximum(ur, 0.5), -1.0)
    # the initial pose: the true one composed with a small motion
    dq = _quat_from_axis_angle(rng.normal(size=3), math.radians(rot_deg))
    q0 = _quat_mul(dq, q_true)
    dt = rng.normal(size=3)
    t0 = rotate(dq, t_true) + dt / np.linalg.norm(dt) * trans
    q0 = (q0 / np.linalg.norm(q0)).astype(dtype)
    t0 = t0.astype(dtype)
    if behind and n:
        Xc0 = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), -5.0])      # camera frame of the INITIAL pose
        q0d = q0.astype(F64)
        Xw[-1] = rotate(q0d * np.array([-1, -1, -1, 1.0]) / np.dot(q0d, q0d), Xc0 - t0.astype(F64))
        planted[-1] = True
    return dict(cam=cam, q=q0, t=t0, xy=xy.astype(dtype), u_right=ur.astype(dtype), inv_sigma2=inv_sigma2.astype(dtype),
                pos_w=Xw.astype(dtype), q_true=q_true, t_true=t_true, planted=planted, median_depth=float(np.median(z)) if n else 1.0)


CAPACITY = 2048     # observations the kernel holds in registers (msorb_pose_optimization_capacity)
WORKGROUP = 256

# name -> make_scene arguments: the scenes of tests/test_pose_opt_gpu.py.  A seed whose chi2 comes within 1e-6 (relative) of a
# threshold under any order is REPLACED here (tests/test_pose_opt_cpu.py::test_threshold_margin asserts, nothing is skipped).
GPU_SCENES = {
    "n0": dict(seed=1, n=0),
    "n2": dict(seed=2, n=2),
    "n3": dict(seed=3, n=3, rot_deg=0.2, trans=0.02),
    "n9": dict(seed=4, n=9, stereo=0.5),
    "n10": dict(seed=5, n=10, stereo=0.5),
    "n63": dict(seed=6, n=63, stereo=0.7, outliers=0.1),
    "n64": dict(seed=7, n=64, stereo=0.7, outliers=0.1),
    "n65": dict(seed=8, n=65, stereo=0.7, outliers=0.1),
    "n255": dict(seed=9, n=WORKGROUP - 1, stereo=0.7, outliers=0.15),
    "n256": dict(seed=10, n=WORKGROUP, stereo=0.7, outliers=0.15),
    "n257": dict(seed=11, n=WORKGROUP + 1, stereo=0.7, outliers=0.15),
    "capacity": dict(seed=12, n=CAPACITY, stereo=0.7, outliers=0.15),
    "capacity_plus_1": dict(seed=13, n=CAPACITY + 1, stereo=0.7, outliers=0.15),
    "n5000": dict(seed=14, n=5000, stereo=0.6, outliers=0.15),
    "all_stereo": dict(seed=15, n=700, stereo=1.0, outliers=0.15),
    "all_mono": dict(seed=16, n=700, stereo=0.0, outliers=0.15),
    "mixed": dict(seed=17, n=1200, stereo=0.5, outliers=0.15),
    "all_outliers": dict(seed=18, n=40, stereo=0.5, garbage=True),
    "rejected_trials": dict(seed=19, n=600, stereo=0.6, outliers=0.4, rot_deg=5.0, trans=0.5),
    "behind": dict(seed=20, n=300, stereo=0.6, outliers=0.1, behind=True),
}
BATCH_SCENES = ("n9", "n65", "n257", "all_mono", "mixed", "all_outliers", "rejected_trials", "behind")   # 8 problems, one call

_scene_cache, _ref_cache = {}, {}


def scene(name):
    if name not in _scene_cache:
        _scene_cache[name] = make_scene(**GPU_SCENES[name])
    return _scene_cache[name]


def reference(name, order="forward"):
    """the restatement's result on a GPU scene, computed once per process"""
    if (name, order) not in _ref_cache:
        s = scene(name)
        _ref_cache[name, order] = pose_optimization(s["cam"], s["q"], s["t"], s["xy"], s["u_right"], s["inv_sigma2"], s["pos_w"], order)
    return _ref_cache[name, order]


def sign_aligned(q, ref):
    q = np.asarray(q, F64)
    return -q if np.dot(q, np.asarray(ref, F64)) < 0 else q


def thresholds(s):
    return np.where(np.asarray(s["u_right"]) >= 0, F64(CHI2_STEREO), F64(CHI2_MONO))


def measure():
    """D: the largest difference between the three orders on qd and on td / median depth, over every GPU scene.
    C: the same on the per-edge chi2 of every classification, relative to max(chi2, threshold).
    margin: the smallest relative distance of any chi2 from its threshold (every scene, round, order)."""
    D = C = 0.0
    margin = math.inf
    per_scene = {}
    for name in GPU_SCENES:
        s = scene(name)
        refs = [reference(name, o) for o in ORDERS]
        th = thresholds(s)
        d = c = 0.0
        for r in refs:
            for chi2 in r["chi2"]:
                with np.errstate(all="ignore"):
                    rel = np.abs(chi2 - th) / th
                if len(rel):
                    margin = min(margin, float(np.nanmin(rel)))
        for a in range(3):
            for b in range(a + 1, 3):
                ra, rb = refs[a], refs[b]
                if s["q"].shape[0] and ra["n_initial"] >= 3:
                    d = max(d, float(np.max(np.abs(sign_aligned(ra["qd"], rb["qd"]) - rb["qd"]))),
                            float(np.max(np.abs(ra["td"] - rb["td"]))) / s["median_depth"])
                for ca, cb in zip(ra["chi2"], rb["chi2"]):
                    with np.errstate(all="ignore"):
                        rel = np.abs(ca - cb) / np.maximum(np.maximum(ca, cb), th)
                    if len(rel):
                        c = max(c, float(np.nanmax(rel)))
        per_scene[name] = dict(D=d, C=c, orders_agree=orders_agree(name))
        D, C = max(D, d), max(C, c)
    return dict(D=D, C=C, pose_bound=16 * D, margin=margin, scenes=per_scene)


def orders_agree(name):
    refs = [reference(name, o) for o in ORDERS]
    return all(r["iterations"] == refs[0]["iterations"] and r["rejected_trials"] == refs[0]["rejected_trials"] for r in refs)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_opt_sensitivity.json")

if __name__ == "__main__":
    if "--measure" in sys.argv:
        m = measure()
        with open(GOLDEN, "w") as f:
            json.dump(m, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps({k: m[k] for k in ("D", "C", "pose_bound", "margin")}))
        for name, v in m["scenes"].items():
            r = reference(name)
            print(f"{name:16s} D={v['D']:.3e} C={v['C']:.3e} agree={v['orders_agree']} it={r['iterations']} rej={r['rejected_trials']} "
                  f"n={r['n_initial']} bad={r['n_bad']}")
    else:
        print(__doc__)
