"""Optimizer::PoseOptimization for a frame with two cameras (the arm src/Optimizer.cc:870-931) or one camera that is not a pinhole,
restated in float64 numpy: the loop of the routine written over an edges object, the edge class of the two cameras
(EdgeSE3ProjectXYZOnlyPose, EdgeSE3ProjectXYZOnlyPoseToBody: include/OptimizableTypes.h:41-45,69-73, src/OptimizableTypes.cpp:49-63,91-107,
src/CameraModels/KannalaBrandt8.cpp:46-65,145-175, Pinhole.cpp:35-41,71-81, g2o/types/se3quat.h:104-110,217-220), a scene generator for
a rig of TUM-VI's geometry and the scene list of the GPU tests.  tests/pose_opt_cases.py gives the shared pieces (rotate, se3_exp,
oplus, solve6, ordered_sum, normalize_rotation); nothing here is shared with ms-slam_amd/csrc/pose_rig_device.h.  No GPU, no library.

`python tests/pose_opt_rig_cases.py --measure` writes tests/golden/pose_opt_rig_sensitivity.json.

KannalaBrandt8::project(Vector3d) takes theta and psi through FLOAT sqrtf / atan2f: here numpy's float32 sqrt (correctly rounded)
and the correctly rounded float arctangent (atan2f below).  A `variant` perturbs what another implementation may round differently:
  order   'forward' | 'reverse' | 'pairwise'   how H, b and the cost are added (pose_opt_cases.ordered_sum)
  dtheta  +1 | -1   theta of project moved one float ulp up / down on every edge
  dpsi    +1 | -1   psi of project likewise
  dfun    +1 | -1   every double atan2 / sin / cos / sqrt of project and projectJac moved one ulp up / down
"""
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_opt_cases as pc  # noqa: E402

F32, F64 = np.float32, np.float64
PINHOLE, KB8 = 0, 1
# a rig of TUM-VI's geometry: 512 x 512 images, KannalaBrandt8 (fx fy cx cy k0 k1 k2 k3), the right camera 10 cm to the right of
# the left one and turned by a degree
IMAGE = 512
CAM_LEFT = (190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504,
            0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182)
CAM_RIGHT = (190.44236969414825, 190.4344384721956, 252.59949716835982, 254.91723064636983,
             0.0034003170790442797, 0.001766278153469831, -0.00266312569781606, 0.0003299517423931039)
CAM_PINHOLE = (458.654, 457.296, 367.215, 248.375)          # a pinhole for the mixed batch (EuRoC's)
TRL_AXIS, TRL_DEG, TRL_T = (0.3, 1.0, 0.2), 1.0, (-0.1, 0.002, 0.001)
VARIANTS = ([dict(order=o) for o in pc.ORDERS] + [dict(dtheta=+1), dict(dtheta=-1), dict(dpsi=+1), dict(dpsi=-1), dict(dfun=+1), dict(dfun=-1)])


def variant_key(v):
    return tuple(sorted((v or {}).items()))


def _ulp(a, d, dtype):
    if not d:
        return a
    return np.nextafter(a, dtype(np.inf if d > 0 else -np.inf), dtype=dtype)


def atan2f(y, x):
    """the float arctangent as the nearest float to the true value: a double arctan2 of the widened arguments, narrowed.  (numpy's
    own float32 arctan2 is a vector routine that is up to 3 ulp off, and glibc's atan2f, which the reference calls, is within one ulp
    of this; the dtheta / dpsi variants cover that ulp.)"""
    assert y.dtype == F32 and x.dtype == F32
    return np.arctan2(y.astype(F64), x.astype(F64)).astype(F32)


def compose(qa, ta, qb, tb):
    """SE3Quat::operator* (se3quat.h:104-110): t = ta + ra * tb, r = ra * rb, normalizeRotation"""
    r = pc.rotate(qa, np.array(tb, F64))
    t = [ta[i] + float(r[i]) for i in range(3)]
    ax, ay, az, aw = qa
    bx, by, bz, bw = qb
    q = [((aw * bx + ax * bw) + ay * bz) - az * by,
         ((aw * by + ay * bw) + az * bx) - ax * bz,
         ((aw * bz + az * bw) + ax * by) - ay * bx,
         ((aw * bw - ax * bx) - ay * by) - az * bz]
    return pc.normalize_rotation(q), t


def rotation_matrix(q):
    """Eigen's Quaternion::toRotationMatrix"""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]


class RigEdges:
    """The edges of :870-931 as arrays.  cams: one or two (type, mvParameters) pairs; camera [n]: 0 = the left camera's edge, 1 = the
    right camera's (to body, through mTrl); obs [n, 2]; w = invSigma2; Xw [n, 3].  Every edge has two rows, deltaMono, chi2Mono."""
    rows = 2

    def __init__(self, cams, q_rl, t_rl, xy, camera, inv_sigma2, pos_w, variant=None):
        v = variant or {}
        self.dtheta, self.dpsi, self.dfun = v.get("dtheta", 0), v.get("dpsi", 0), v.get("dfun", 0)
        self.right = np.asarray(camera).reshape(-1) != 0
        par = []
        for kind, p in cams:
            a = np.zeros(8, F32)
            a[:len(p)] = np.asarray(p, F32)            # mvParameters are floats
            par.append((kind, a.astype(F64)))          # widened where they are used
        if len(par) == 1:
            par.append(par[0])
        self.kind = np.where(self.right, par[1][0], par[0][0])
        self.p = [np.where(self.right, par[1][1][k], par[0][1][k]) for k in range(8)]
        self.p32 = [np.where(self.right, F32(par[1][1][k]), F32(par[0][1][k])).astype(F32) for k in range(8)]
        if q_rl is None:
            q_rl, t_rl = (0, 0, 0, 1), (0, 0, 0)
        self.q_rl = pc.normalize_rotation(np.asarray(q_rl, F32).astype(F64))     # SE3Quat(q, t) normalises (Optimizer.cc:923)
        self.t_rl = [float(c) for c in np.asarray(t_rl, F32).astype(F64)]
        self.R_rl = rotation_matrix(self.q_rl)
        self.x = np.asarray(xy, F64).reshape(-1, 2)[:, 0]
        self.y = np.asarray(xy, F64).reshape(-1, 2)[:, 1]
        self.w = np.asarray(inv_sigma2, F64).reshape(-1)
        self.Xw = np.asarray(pos_w, F64).reshape(-1, 3)
        self.n = len(self.w)
        self.stereo = np.zeros(self.n, bool)
        self.delta = np.full(self.n, pc.DELTA_MONO)
        self.th = np.full(self.n, pc.CHI2_MONO, F32)

    def _fun(self, a):
        return _ulp(a, self.dfun, F64)

    def project(self, P):
        """pCamera->project(Vector3d) of each edge's own camera"""
        x, y, z = P[:, 0], P[:, 1], P[:, 2]
        p = self.p
        pu = (p[0] * x) / z + p[2]                                            # Pinhole.cpp:35-41
        pv = (p[1] * y) / z + p[3]
        x2_plus_y2 = x * x + y * y                                            # KannalaBrandt8.cpp:46-65
        theta = atan2f(np.sqrt(x2_plus_y2.astype(F32)), z.astype(F32))        # atan2f(sqrtf(.), .)
        psi = atan2f(y.astype(F32), x.astype(F32))
        assert theta.dtype == F32 and psi.dtype == F32
        theta = _ulp(theta, self.dtheta, F32).astype(F64)
        psi = _ulp(psi, self.dpsi, F32).astype(F64)
        theta2 = theta * theta
        theta3 = theta * theta2
        theta5 = theta3 * theta2
        theta7 = theta5 * theta2
        theta9 = theta7 * theta2
        r = (((theta + p[4] * theta3) + p[5] * theta5) + p[6] * theta7) + p[7] * theta9
        ku = (p[0] * r) * self._fun(np.cos(psi)) + p[2]
        kv = (p[1] * r) * self._fun(np.sin(psi)) + p[3]
        pin = self.kind == PINHOLE
        return np.where(pin, pu, ku), np.where(pin, pv, kv)

    def project_jac(self, P):
        """pCamera->projectJac(Vector3d) -> [n, 2, 3]"""
        x, y, z = P[:, 0], P[:, 1], P[:, 2]
        p, p32 = self.p, self.p32
        Jp = np.zeros((self.n, 2, 3), F64)                                    # Pinhole.cpp:71-81
        Jp[:, 0, 0] = p[0] / z
        Jp[:, 0, 2] = (-p[0] * x) / (z * z)
        Jp[:, 1, 1] = p[1] / z
        Jp[:, 1, 2] = (-p[1] * y) / (z * z)
        x2, y2, z2 = x * x, y * y, z * z                                      # KannalaBrandt8.cpp:145-175
        r2 = x2 + y2
        r = self._fun(np.sqrt(r2))
        r3 = r2 * r
        theta = self._fun(np.arctan2(r, z))
        theta2 = theta * theta
        theta3 = theta2 * theta
        theta4 = theta2 * theta2
        theta5 = theta4 * theta
        theta6 = theta2 * theta4
        theta7 = theta6 * theta
        theta8 = theta4 * theta4
        theta9 = theta8 * theta
        f = (((theta + theta3 * p[4]) + theta5 * p[5]) + theta7 * p[6]) + theta9 * p[7]
        k3, k5, k7, k9 = ((F32(m) * p32[i]).astype(F64) for m, i in ((3, 4), (5, 5), (7, 6), (9, 7)))   # int * float: a float product
        fd = (((1 + k3 * theta2) + k5 * theta4) + k7 * theta6) + k9 * theta8
        den = r2 * (r2 + z2)
        K = np.empty((self.n, 2, 3), F64)
        K[:, 0, 0] = p[0] * (((fd * z) * x2) / den + (f * y2) / r3)
        K[:, 1, 0] = p[1] * ((((fd * z) * y) * x) / den - ((f * y) * x) / r3)
        K[:, 0, 1] = p[0] * ((((fd * z) * y) * x) / den - ((f * y) * x) / r3)
        K[:, 1, 1] = p[1] * (((fd * z) * y2) / den + (f * x2) / r3)
        K[:, 0, 2] = ((-p[0] * fd) * x) / (r2 + z2)
        K[:, 1, 2] = ((-p[1] * fd) * y) / (r2 + z2)
        return np.where((self.kind == PINHOLE)[:, None, None], Jp, K)

    def error(self, q, t):
        """computeError of both edges -> e [n, 2], X_l = T.map(Xw) [n, 3], chi2 [n] (base_edge.h:60)"""
        with np.errstate(all="ignore"):
            Xl = pc.rotate(q, self.Xw) + np.array(t, F64)                     # SE3Quat::map
            q_rw, t_rw = compose(self.q_rl, self.t_rl, q, t)                  # mTrl * estimate
            Xr = pc.rotate(q_rw, self.Xw) + np.array(t_rw, F64)
            u, v = self.project(np.where(self.right[:, None], Xr, Xl))
            e = np.stack([self.x - u, self.y - v], -1)
            chi2 = e[:, 0] * (self.w * e[:, 0]) + e[:, 1] * (self.w * e[:, 1])
        return e, Xl, chi2

    def jacobian(self, Xl):
        """linearizeOplus of both edges -> [n, 2, 6]"""
        with np.errstate(all="ignore"):
            Xr = pc.rotate(self.q_rl, Xl) + np.array(self.t_rl, F64)          # mTrl.map(T_lw.map(Xw))
            Jp = self.project_jac(np.where(self.right[:, None], Xr, Xl))
            R = self.R_rl
            A = -Jp
            AR = np.empty_like(A)
            for i in range(2):
                for j in range(3):
                    AR[:, i, j] = (A[:, i, 0] * R[0][j] + A[:, i, 1] * R[1][j]) + A[:, i, 2] * R[2][j]
            A = np.where(self.right[:, None, None], AR, A)
            x, y, z = Xl[:, 0], Xl[:, 1], Xl[:, 2]
            J = np.empty((self.n, 2, 6), F64)                                 # times SE3deriv = [0 z -y 1 0 0; -z 0 x 0 1 0; y -x 0 0 0 1]
            for i in range(2):
                J[:, i, 0] = A[:, i, 1] * -z + A[:, i, 2] * y
                J[:, i, 1] = A[:, i, 0] * z + A[:, i, 2] * -x
                J[:, i, 2] = A[:, i, 0] * -y + A[:, i, 1] * x
                J[:, i, 3], J[:, i, 4], J[:, i, 5] = A[:, i, 0], A[:, i, 1], A[:, i, 2]
        return J

    def huber(self, chi2, robust):
        """RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91) -> rho, rho'"""
        if not robust:
            return chi2, np.ones_like(chi2)
        with np.errstate(all="ignore"):
            dsqr = self.delta * self.delta
            inl = chi2 <= dsqr
            s = np.sqrt(chi2)
            return np.where(inl, chi2, (2 * s) * self.delta - dsqr), np.where(inl, 1.0, self.delta / s)


def optimize(E, q, t, sum_order="forward"):
    """Optimizer.cc:936-1037 with g2o's Levenberg loop (optimization_algorithm_levenberg.cpp:61-195, sparse_optimizer.cpp:354-419) over
    the edges object E (n, rows, w, th, error, jacobian, huber) -> the dict of pose_opt_cases.pose_optimization"""
    n = E.n
    res = dict(n_initial=n, iterations=[-1] * 4, rejected_trials=[-1] * 4, chi2=[], flags=[], outlier=np.zeros(n, bool))
    qf, tf = np.asarray(q, F32), np.asarray(t, F32)
    if n < 3:                                              # :936-937
        res.update(q=qf.copy(), t=tf.copy(), qd=qf.astype(F64), td=tf.astype(F64), n_bad=n)
        return res
    q0, t0 = pc.normalize_rotation(qf.astype(F64)), [float(v) for v in tf.astype(F64)]   # :774-775
    level = np.zeros(n, bool)
    chi2_state = np.zeros(n, F64)
    x = [0.0] * 6
    n_bad = 0
    for it in range(4):                                    # :946
        robust = it < 3                                    # :974-975, :998-999
        cq, ct = list(q0), list(t0)                        # :947-948
        n_solve = n_rejected = 0
        act = ~level
        if act.any():                                      # sparse_optimizer.cpp:356-359
            lam, ni, n_bad_steps, ok, i = 0.0, 2.0, 0, True, 0
            while i < 10 and ok:                           # sparse_optimizer.cpp:376
                e, p, chi2 = E.error(cq, ct)               # levenberg.cpp:75
                chi2_state[act] = chi2[act]
                rho0, rho1 = E.huber(chi2, robust)
                J = E.jacobian(p)                          # :87 buildSystem (base_unary_edge.hpp:43-72)
                w = E.w
                wr = rho1 * w                              # robustInformation (base_edge.h:96-100)
                terms = np.empty((n, 28), F64)
                k = 0
                with np.errstate(all="ignore"):
                    for a in range(6):
                        for c in range(a, 6):
                            tt = (J[:, 0, a] * wr) * J[:, 0, c]
                            for r in range(1, E.rows):
                                tt = tt + (J[:, r, a] * wr) * J[:, r, c]
                            terms[:, k] = tt
                            k += 1
                        tt = ((rho1 * J[:, 0, a]) * w) * e[:, 0]
                        for r in range(1, E.rows):
                            tt = tt + ((rho1 * J[:, r, a]) * w) * e[:, r]
                        terms[:, 21 + a] = -tt
                    terms[:, 27] = rho0                    # activeRobustChi2 (:82)
                S = pc.ordered_sum(terms[act], sum_order)
                Hu, b = S[:21], S[21:27]
                current = float(S[27])
                ini = current
                if i == 0:                                 # computeLambdaInit (:172-186)
                    max_diag, kk = 0.0, 0
                    for j in range(6):
                        max_diag = max(abs(float(Hu[kk])), max_diag)
                        kk += 6 - j
                    lam, ni, n_bad_steps = 1e-5 * max_diag, 2.0, 0
                rho, qmax = 0.0, 0
                while True:
                    bq, bt = list(cq), list(ct)            # push (:103)
                    ok2 = pc.solve6(Hu, lam, b, x)         # :109-110
                    cq, ct = pc.oplus(cq, ct, x)           # :115
                    _, _, chi2 = E.error(cq, ct)           # :123
                    chi2_state[act] = chi2[act]
                    r0, _ = E.huber(chi2, robust)
                    temp = float(pc.ordered_sum(r0[act][:, None], sum_order)[0])   # :124
                    if not ok2:
                        temp = pc.DBL_MAX                  # :126-127
                    with np.errstate(all="ignore"):
                        rho = F64(current) - F64(temp)
                        scale = 0.0                        # computeScale (:188-195)
                        for j in range(6):
                            scale += x[j] * (lam * x[j] + float(b[j]))
                        scale += 1e-3
                        rho = float(rho / F64(scale))
                    if rho > 0 and math.isfinite(temp):    # :134-142
                        yy = 2 * rho - 1
                        alpha = min(1. - (yy * yy) * yy, 2. / 3.)
                        lam *= max(1. / 3., alpha)
                        ni = 2.0
                        current = temp
                    else:                                  # :143-147
                        lam *= ni
                        ni *= 2
                        cq, ct = bq, bt
                        n_rejected += 1
                    qmax += 1
                    if not (rho < 0 and qmax < 10):        # :149
                        break
                n_solve += 1
                i += 1
                if qmax == 10 or rho == 0:                 # :151-155
                    ok = False
                    continue
                if (ini - current) * 1e3 < ini:            # :157-162
                    n_bad_steps += 1
                else:
                    n_bad_steps = 0
                if n_bad_steps >= 3:                       # :164-167
                    ok = False
        res["iterations"][it], res["rejected_trials"][it] = n_solve, n_rejected
        _, _, fresh = E.error(cq, ct)                      # :959-961, :983-985: only the current outliers are recomputed
        chi2_state[level] = fresh[level]
        res["chi2"].append(chi2_state.copy())
        with np.errstate(all="ignore"):
            level = chi2_state.astype(F32) > E.th          # :963-972, :987-996
        res["flags"].append(level.copy())
        n_bad = int(level.sum())
        if n < 10:                                         # :1026-1027
            break
    res.update(qd=np.array(cq, F64), td=np.array(ct, F64), n_bad=n_bad, outlier=level.copy())
    res["q"], res["t"] = res["qd"].astype(F32), res["td"].astype(F32)   # :1033-1034
    return res


def pose_optimization_rig(s, variant=None):
    """the routine on a scene dict (make_rig_scene)"""
    E = RigEdges(s["cams"], s["q_rl"], s["t_rl"], s["xy"], s["camera"], s["inv_sigma2"], s["pos_w"], variant)
    return optimize(E, s["q"], s["t"], (variant or {}).get("order", "forward"))


# ------------------------------------------------------------------------------------------------------------ scenes
def trl():
    """-> q_rl, t_rl (float32): what GetRelativePoseTrl() holds"""
    return pc._quat_from_axis_angle(TRL_AXIS, math.radians(TRL_DEG)).astype(F32), np.array(TRL_T, F32)


def make_rig_scene(seed, n, right=0.5, interleaved=False, cams=("kb8", "kb8"), outliers=0.0, noise=0.4, rot_deg=1.0, trans=0.05,
                   theta_deg=(1.0, 75.0), garbage=False):
    """A random pose and n points on rays of the camera that sees them: theta drawn over theta_deg, psi over the circle, 1-10 m away,
    projected with the restatement's own project, noise sigma px at level 0 (times the level's scale), a share `outliers` moved by
    20-200 px.  right: share of the observations made by the right camera; they follow the left ones unless `interleaved`.
    cams: 'kb8' | 'pinhole' per camera, one entry for a one-camera frame.  garbage: every observation unrelated to its point.
    -> dict(cams, n_cameras, q_rl, t_rl (None with one camera), q, t, xy, camera, inv_sigma2, pos_w, planted, median_depth)"""
    rng = np.random.default_rng(seed)
    table = {"kb8": (KB8, CAM_LEFT), "kb8r": (KB8, CAM_RIGHT), "pinhole": (PINHOLE, CAM_PINHOLE)}
    names = list(cams)
    if len(names) == 2 and names[1] == "kb8":
        names[1] = "kb8r"
    cam_list = [(table[c][0], np.asarray(table[c][1], F32)) for c in names]
    two = len(cam_list) == 2
    q_rl, t_rl = trl() if two else (None, None)
    camera = (rng.uniform(size=n) < right).astype(np.uint8) if two else np.zeros(n, np.uint8)
    if not interleaved:
        camera = np.sort(camera)
    q_true = pc._quat_from_axis_angle(rng.normal(size=3), math.radians(rng.uniform(0, 30)))
    t_true = rng.uniform(-1, 1, 3)
    theta = np.radians(rng.uniform(theta_deg[0], theta_deg[1], n))
    for c, nm in enumerate(names):                      # a pinhole sees less
        if nm == "pinhole":
            theta = np.where(camera == c, np.radians(rng.uniform(1.0, 35.0, n)), theta)
    psi = rng.uniform(-math.pi, math.pi, n)
    depth = rng.uniform(1, 10, n)
    Xc = np.stack([np.sin(theta) * np.cos(psi), np.sin(theta) * np.sin(psi), np.cos(theta)], -1) * depth[:, None]   # in the seeing camera
    levels = rng.integers(0, 8, n)
    sigma = 1.2 ** levels
    inv_sigma2 = (1.0 / (sigma * sigma)).astype(F32)
    E0 = RigEdges(cam_list, None, None, np.zeros((n, 2)), camera, inv_sigma2, Xc)
    u, v = E0.project(Xc) if n else (np.zeros(0), np.zeros(0))            # each point through its own camera
    xy = np.stack([u, v], -1) + rng.normal(size=(n, 2)) * (noise * sigma)[:, None]
    planted = rng.uniform(size=n) < outliers
    ang, mag = rng.uniform(0, 2 * math.pi, n), rng.uniform(20, 200, n)
    xy[planted] += (np.stack([np.cos(ang), np.sin(ang)], -1) * mag[:, None])[planted]
    if garbage:
        xy = rng.uniform(0, IMAGE, (n, 2))
        planted[:] = True
    Xl = Xc.copy()
    if two and n:
        qd, td = pc.normalize_rotation(q_rl.astype(F64)), t_rl.astype(F64)
        inv = np.array(qd) * np.array([-1, -1, -1, 1.0])
        Xl = np.where((camera != 0)[:, None], pc.rotate(inv, Xc - td), Xc)
    Xw = pc.rotate(q_true * np.array([-1, -1, -1, 1.0]), Xl - t_true) if n else np.zeros((0, 3))
    dq = pc._quat_from_axis_angle(rng.normal(size=3), math.radians(rot_deg))
    q0 = pc._quat_mul(dq, q_true)
    dt = rng.normal(size=3)
    t0 = pc.rotate(dq, t_true) + dt / np.linalg.norm(dt) * trans
    return dict(cams=cam_list, n_cameras=len(cam_list), q_rl=q_rl, t_rl=t_rl, q=(q0 / np.linalg.norm(q0)).astype(F32), t=t0.astype(F32),
                xy=xy.astype(F32), camera=camera, inv_sigma2=inv_sigma2, pos_w=Xw.astype(F32), planted=planted,
                median_depth=float(np.median(depth)) if n else 1.0)


CAPACITY = 2048     # observations the rig kernel holds in registers (msorb_pose_optimization_rig_capacity)
WORKGROUP = 256

# name -> make_rig_scene arguments: the scenes of tests/test_pose_opt_rig_gpu.py.  A seed on which the variants disagree on a flag, or
# on which a chi2 comes within 16 C of its threshold (tests/test_pose_opt_rig_cpu.py::test_threshold_margin), is REPLACED here.
GPU_SCENES = {
    "n2": dict(seed=2, n=2),
    "n3": dict(seed=3, n=3, rot_deg=0.2, trans=0.01),
    "n9": dict(seed=4, n=9),
    "n10": dict(seed=5, n=10),
    "n63": dict(seed=6, n=63, outliers=0.1),
    "n64": dict(seed=7, n=64, outliers=0.1),
    "n65": dict(seed=8, n=65, outliers=0.1),
    "n255": dict(seed=9, n=WORKGROUP - 1, outliers=0.15),
    "n256": dict(seed=10, n=WORKGROUP, outliers=0.15),
    "n257": dict(seed=11, n=WORKGROUP + 1, outliers=0.15),
    "capacity": dict(seed=12, n=CAPACITY, outliers=0.15),
    "capacity_plus_1": dict(seed=13, n=CAPACITY + 1, outliers=0.15),
    "fisheye_mono": dict(seed=14, n=700, cams=("kb8",), outliers=0.15),
    "right_only": dict(seed=15, n=700, right=1.0, outliers=0.15),
    "rig": dict(seed=16, n=1200, outliers=0.15),
    "rig_interleaved": dict(seed=16, n=1200, outliers=0.15, interleaved=True),
    "wide": dict(seed=17, n=300, outliers=0.1, theta_deg=(1.0, 100.0)),
    "all_outliers": dict(seed=18, n=40, garbage=True),
    "rejected_trials": dict(seed=19, n=600, outliers=0.4, rot_deg=5.0, trans=0.3),
    "pinhole_left": dict(seed=20, n=150, cams=("pinhole", "kb8"), outliers=0.1),
}
BATCH_SCENES = ("n9", "n65", "fisheye_mono", "rig_interleaved", "wide", "capacity_plus_1", "pinhole_left", "all_outliers")   # 8, one call
CPU_SUBSET = ("n10", "n65", "n257", "fisheye_mono", "wide", "pinhole_left")   # re-measured by tests/test_pose_opt_rig_cpu.py

_scene_cache, _ref_cache = {}, {}


def scene(name):
    if name not in _scene_cache:
        _scene_cache[name] = make_rig_scene(**GPU_SCENES[name])
    return _scene_cache[name]


def reference(name, variant=None):
    """the restatement's result on a GPU scene under a variant (None = 'forward', unperturbed), computed once per process"""
    key = (name, variant_key(variant if variant and variant != dict(order="forward") else None))
    if key not in _ref_cache:
        _ref_cache[key] = pose_optimization_rig(scene(name), variant)
    return _ref_cache[key]


def variants_agree(name):
    """iterations and rejected trials are the same under every variant"""
    refs = [reference(name, v) for v in VARIANTS]
    return all(r["iterations"] == refs[0]["iterations"] and r["rejected_trials"] == refs[0]["rejected_trials"] for r in refs)


def flags_agree(name):
    """every variant gives every edge the same flag at every classification"""
    refs = [reference(name, v) for v in VARIANTS]
    return all(len(r["flags"]) == len(refs[0]["flags"]) and all(np.array_equal(a, b) for a, b in zip(r["flags"], refs[0]["flags"]))
               for r in refs)


def measure_scene(name):
    """-> D (pose: qd, td / median depth), C (per-edge chi2 relative to max(chi2, threshold)): the spread over VARIANTS;
    margin: the smallest relative distance of any chi2 from its threshold (every round, every variant)"""
    s = scene(name)
    refs = [reference(name, v) for v in VARIANTS]
    th = F64(pc.CHI2_MONO)
    d = c = 0.0
    margin = math.inf
    if refs[0]["n_initial"] >= 3:
        qs = np.stack([pc.sign_aligned(r["qd"], refs[0]["qd"]) for r in refs])
        ts = np.stack([r["td"] for r in refs])
        d = max(float(np.max(qs.max(0) - qs.min(0))), float(np.max(ts.max(0) - ts.min(0))) / s["median_depth"])
        for rnd in range(min(len(r["chi2"]) for r in refs)):
            ch = np.stack([r["chi2"][rnd] for r in refs])
            with np.errstate(all="ignore"):
                rel = (ch.max(0) - ch.min(0)) / np.maximum(ch.max(0), th)
                c = max(c, float(np.nanmax(rel)))
                margin = min(margin, float(np.nanmin(np.abs(ch - th) / th)))
    return dict(D=d, C=c, margin=margin if math.isfinite(margin) else None, variants_agree=variants_agree(name), flags_agree=flags_agree(name))


def measure(names=None):
    per = {name: measure_scene(name) for name in (names or GPU_SCENES)}
    D, C = max(v["D"] for v in per.values()), max(v["C"] for v in per.values())
    return dict(D=D, C=C, pose_bound=16 * D, margin_needed=16 * C, margin=min(v["margin"] for v in per.values() if v["margin"] is not None), scenes=per)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_opt_rig_sensitivity.json")

# ------------------------------------------------------------------------- the files of tests/pose_opt_rig_main.cc (include/msorb.h's records)
CAMERA_DTYPE = np.dtype([("type", "<i4"), ("p", "<f4", 8)])
PROBLEM_DTYPE = np.dtype([("q", "<f4", 4), ("t", "<f4", 3), ("n_cameras", "<i4"), ("cam", CAMERA_DTYPE, 2), ("q_rl", "<f4", 4),
                          ("t_rl", "<f4", 3), ("n", "<i4")])
RESULT_DTYPE = np.dtype([("q", "<f4", 4), ("t", "<f4", 3), ("_pad", "<i4"), ("qd", "<f8", 4), ("td", "<f8", 3), ("n_initial", "<i4"),
                         ("n_bad", "<i4"), ("iterations", "<i4", 4), ("rejected_trials", "<i4", 4)])
assert PROBLEM_DTYPE.itemsize == 136 and RESULT_DTYPE.itemsize == 128


def problem_record(s):
    p = np.zeros(1, PROBLEM_DTYPE)
    p["q"], p["t"], p["n"], p["n_cameras"] = s["q"], s["t"], len(s["camera"]), s["n_cameras"]
    for c, (kind, par) in enumerate(s["cams"]):
        p["cam"][0, c]["type"] = kind
        p["cam"][0, c]["p"][:len(par)] = par
    if s["q_rl"] is not None:
        p["q_rl"], p["t_rl"] = s["q_rl"], s["t_rl"]
    return p


def write_problem(path, s):
    """problem record | xy | camera | inv_sigma2 | pos_w"""
    with open(path, "wb") as f:
        f.write(problem_record(s).tobytes())
        f.write(np.ascontiguousarray(s["xy"], "<f4").tobytes())
        f.write(np.ascontiguousarray(s["camera"], np.uint8).tobytes())
        f.write(np.ascontiguousarray(s["inv_sigma2"], "<f4").tobytes())
        f.write(np.ascontiguousarray(s["pos_w"], "<f4").tobytes())


def read_result(path, n):
    blob = open(path, "rb").read()
    assert len(blob) == 128 + n
    return np.frombuffer(blob, RESULT_DTYPE, 1)[0], np.frombuffer(blob, np.uint8, n, 128).astype(bool)


if __name__ == "__main__":
    if "--measure" in sys.argv:
        m = measure()
        with open(GOLDEN, "w") as f:
            json.dump(m, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps({k: m[k] for k in ("D", "C", "pose_bound", "margin_needed", "margin")}))
        for name, v in m["scenes"].items():
            r = reference(name)
            print(f"{name:16s} D={v['D']:.3e} C={v['C']:.3e} margin={v['margin']} agree={v['variants_agree']} flags={v['flags_agree']} "
                  f"it={r['iterations']} rej={r['rejected_trials']} n={r['n_initial']} bad={r['n_bad']}")
    else:
        print(__doc__)
