"""The shared Lie-group primitives one at a time (msorb_debug_lie, ms-slam_amd/csrc/lie_probe_device.h): the records of every
function, the exact value of each record, the float64 / float32 variants and the sensitivity D(function, family).

The exact value is the REFERENCE'S FORMULA, branch by branch, in mpmath at 60 digits on the double (or float) inputs as they are:
where the reference is itself inexact (the second-order small-angle R, LogSO3's unscaled early exits, Sim3::log's small-angle B) the
exact value is that branch in high precision.  The polar factor of ExpSO3, NormalizeRotation and MLPnP's U V^T is U V^T of
mpmath.svd_r.  A double the reference STORES before the function reads it stays a double (RobustKernelHuber's dsqr of setDelta, the
bias narrowed to float).

One text serves the exact value and the restatements the project did not have yet (Sim3::log, the two Rodrigues maps, the bias
correction, the 3x3 LU, Huber): every g_* below is written over an arithmetic `A` that is mpmath, float64 or float32, the last two
with the project's one-ulp nudge of every libm result.  The variants of the sensitivity are those plus the restatements of
inertial_opt_cases.py, pose_opt_cases.py and sim3_opt_cases.py, imported.

Every comparison a function makes goes through A.cmp, which records its outcome and, in mpmath, its margin.  The condition on the
inputs (tests/test_lie_primitives_cpu.py): every float run takes the branches of the exact run, and every margin is above MARGIN_MIN
unless the record is one of those whose predicate is decided in exact arithmetic (`decided`: the axis-aligned threshold records,
the exact edge matrices, the LU ties).

    python tests/lie_primitives_cases.py --write-golden     writes tests/golden/lie_primitives_sensitivity.json
"""
import functools
import json
import math
import os
import struct
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inertial_opt_cases as ic   # noqa: E402
import pose_opt_cases as pc       # noqa: E402
import sim3_opt_cases as sc3      # noqa: E402

mp.mp.dps = 60
F32, F64 = np.float32, np.float64
MARGIN = 16                       # one more order and another libm
MARGIN_MIN = 2.0 ** -44           # 256 ulps: the operands of a float64 run are a few ulps (2^-53) from the exact ones
MARGIN_MIN_F32 = 2.0 ** -18       # 64 ulps of the float chain (2^-24)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lie_primitives_sensitivity.json")
LIE_IN, LIE_OUT = 16, 24
OPS = ("rotate", "normalize_rotation", "quaternion_of_matrix", "se3_exp", "oplus", "huber", "sim3_exp", "sim3_mul", "sim3_inverse",
       "lu3_solve", "sim3_log", "normalize_rotation_eg4", "exp_so3", "log_so3", "normalize_rotation_f", "so3f_exp_matrix",
       "bias_corrected", "right_jacobian_so3", "inverse_right_jacobian_so3", "mlpnp_nearest_rotation", "mlpnp_rodrigues2rot",
       "mlpnp_rot2rodrigues")
N_OUT = dict(rotate=3, normalize_rotation=4, quaternion_of_matrix=4, se3_exp=7, oplus=7, huber=2, sim3_exp=8, sim3_mul=8, sim3_inverse=8,
             lu3_solve=3, sim3_log=7, normalize_rotation_eg4=9, exp_so3=9, log_so3=3, normalize_rotation_f=9, so3f_exp_matrix=9,
             bias_corrected=18, right_jacobian_so3=9, inverse_right_jacobian_so3=9, mlpnp_nearest_rotation=9, mlpnp_rodrigues2rot=9,
             mlpnp_rot2rodrigues=3)
FLOAT_CHAIN = ("normalize_rotation_f", "so3f_exp_matrix", "bias_corrected")
# no libm call other than sqrt in any branch: the device equals the host program bit for bit
LIBM_FREE = ("rotate", "normalize_rotation", "quaternion_of_matrix", "huber", "sim3_mul", "sim3_inverse", "lu3_solve",
             "normalize_rotation_eg4", "normalize_rotation_f", "mlpnp_nearest_rotation")
# ... and the small-angle arms of these (family "small")
LIBM_FREE_SMALL = ("se3_exp", "exp_so3", "right_jacobian_so3", "inverse_right_jacobian_so3", "so3f_exp_matrix")


def in_width(fn):
    return LIE_IN * (5 if fn == "bias_corrected" else 1)


def bits_bound(fn, family, D):
    """True: bit equality with the host program is this family's bound (section 3 of the issue, first kind)"""
    return fn in LIBM_FREE or (fn in LIBM_FREE_SMALL and family.startswith("small")) or D == 0.0


# ------------------------------------------------------------------------------------------------------------ arithmetics
class Arith:
    """kind 'mp' (exact), 'f64' or 'f32'; nudge: every libm result one ulp up; ortho: how a float run takes the polar factor
    ('svd', 'polar' = Newton, 'jacobi' = the one-sided Jacobi the headers state)"""

    def __init__(self, kind, nudge=False, ortho="jacobi"):
        self.kind, self.nudge, self.ortho = kind, nudge, ortho
        self.trace, self.margins = [], []
        self.T = {"mp": mp.mpf, "f64": F64, "f32": F32}[kind]

    def k(self, x):
        return mp.mpf(float(x)) if self.kind == "mp" else self.T(x)

    def narrow32(self, x):
        """a double the reference narrows to float before it computes"""
        return self.k(float(F32(float(x))))

    def round64(self, x):
        """a value the reference stores in a double before the function reads it"""
        return self.k(float(x))

    def fn(self, name, x):
        if self.kind == "mp":
            if name == "acos" and not (-1 <= x <= 1):
                return mp.nan                                  # glibc's and OCML's acos of an argument outside [-1, 1]
            return getattr(mp, name)(x)
        with np.errstate(all="ignore"):
            v = getattr(np, {"acos": "arccos"}.get(name, name))(x)
        if self.nudge and not (name == "exp" and x == 0):      # exp(0) is 1 in every libm (sim3_opt_cases.sim3_exp)
            v = np.nextafter(v, self.T(np.inf))
        return self.T(v)

    def sqrt(self, x):
        return mp.sqrt(x) if self.kind == "mp" else self.T(np.sqrt(x))

    def div(self, a, b):
        if self.kind != "mp":
            with np.errstate(all="ignore"):
                return self.T(a) / self.T(b)
        if b == 0:
            return mp.nan if (a == 0 or mp.isnan(a)) else (mp.inf if a > 0 else -mp.inf)
        return a / b

    def cmp(self, tag, a, op, b, scale=None, inputs=False):
        """the comparison a <op> b.  scale: the natural magnitude of the operands where one of them is 0; inputs: both operands
        are inputs of the function, which every arithmetic holds exactly"""
        r = bool({"<": a < b, ">": a > b, "<=": a <= b, ">=": a >= b}[op])
        self.trace.append((tag, r))
        if self.kind == "mp":
            if inputs or mp.isnan(a) or mp.isnan(b) or mp.isinf(a) or mp.isinf(b):
                m = math.inf
            else:
                s = max(abs(a), abs(b)) if scale is None else max(abs(a), abs(b), mp.mpf(scale))
                m = float(abs(a - b) / s) if s > 0 else 0.0
            self.margins.append((tag, m))
        return r


def EXACT():
    return Arith("mp")


# -------------------------------------------------------------------------------------------- the functions over an arithmetic
def _eye(A):
    return [[A.k(1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]


def _skew(A, x, y, z):
    o = A.k(0.0)
    return [[o, -z, y], [z, o, -x], [-y, x, o]]


def _mm(X, Y):
    return [[(X[i][0] * Y[0][j] + X[i][1] * Y[1][j]) + X[i][2] * Y[2][j] for j in range(3)] for i in range(3)]


def _mv(X, v):
    return [(X[i][0] * v[0] + X[i][1] * v[1]) + X[i][2] * v[2] for i in range(3)]


def _m33(a):
    return [list(a[0:3]), list(a[3:6]), list(a[6:9])]


def _flat(M):
    return [M[i][j] for i in range(3) for j in range(3)]


def g_rotate(A, q, v):
    qx, qy, qz, qw = q
    X, Y, Z = v
    ux, uy, uz = qy * Z - qz * Y, qz * X - qx * Z, qx * Y - qy * X
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return [(X + qw * ux) + (qy * uz - qz * uy), (Y + qw * uy) + (qz * ux - qx * uz), (Z + qw * uz) + (qx * uy - qy * ux)]


def g_normalize_q(A, q, inputs=False):
    """se3quat.h:280-285"""
    q = list(q)
    if A.cmp("qw<0", q[3], "<", A.k(0.0), scale=1.0, inputs=inputs):
        q = [c * A.k(-1.0) for c in q]
    n = A.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [A.div(c, n) for c in q]


def g_qom(A, R, inputs=False):
    """Quaterniond(Matrix3d), Eigen/src/Geometry/Quaternion.h"""
    q = [None] * 4
    half, one = A.k(0.5), A.k(1.0)
    t = (R[0][0] + R[1][1]) + R[2][2]
    if A.cmp("trace>0", t, ">", A.k(0.0), scale=1.0):
        t = A.sqrt(t + one)
        q[3] = half * t
        t = A.div(half, t)
        q[0], q[1], q[2] = (R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t
    else:
        i = 0
        if A.cmp("R11>R00", R[1][1], ">", R[0][0], scale=1.0, inputs=inputs):
            i = 1
        if A.cmp("R22>Rii", R[2][2], ">", R[i][i], scale=1.0, inputs=inputs):
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = A.sqrt(((R[i][i] - R[j][j]) - R[k][k]) + one)
        q[i] = half * t
        t = A.div(half, t)
        q[3] = (R[k][j] - R[j][k]) * t
        q[j] = (R[j][i] + R[i][j]) * t
        q[k] = (R[k][i] + R[i][k]) * t
    return q


def g_se3_exp(A, u):
    """SE3Quat::exp (se3quat.h:223-257)"""
    ox, oy, oz = u[0:3]
    theta = A.sqrt((ox * ox + oy * oy) + oz * oz)
    O = _skew(A, ox, oy, oz)
    O2, I = _mm(O, O), _eye(A)
    if A.cmp("theta<1e-5", theta, "<", A.k(0.00001)):
        R = [[(I[i][j] + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
        V = R
    else:
        s, c = A.fn("sin", theta), A.fn("cos", theta)
        a, b, d = A.div(s, theta), A.div(A.k(1.0) - c, theta * theta), A.div(theta - s, (theta * theta) * theta)
        R = [[(I[i][j] + a * O[i][j]) + b * O2[i][j] for j in range(3)] for i in range(3)]
        V = [[(I[i][j] + b * O[i][j]) + d * O2[i][j] for j in range(3)] for i in range(3)]
    return g_normalize_q(A, g_qom(A, R)) + _mv(V, u[3:6])


def g_oplus(A, T, x):
    """VertexSE3Expmap::oplusImpl: exp(x) * T (se3quat.h:104-110)"""
    E = g_se3_exp(A, x)
    ex, ey, ez, ew = E[0:4]
    tx, ty, tz, tw = T[0:4]
    r = g_rotate(A, E[0:4], T[4:7])
    q = [((ew * tx + ex * tw) + ey * tz) - ez * ty, ((ew * ty + ey * tw) + ez * tx) - ex * tz,
         ((ew * tz + ez * tw) + ex * ty) - ey * tx, ((ew * tw - ex * tx) - ey * ty) - ez * tz]
    return g_normalize_q(A, q) + [E[4 + i] + r[i] for i in range(3)]


def g_huber(A, chi2, delta, robust):
    """RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91); dsqr is the double setDelta stored (:65-69)"""
    if not robust:
        return [chi2, A.k(1.0)]
    dsqr = A.round64(delta * delta)
    if A.cmp("chi2<=dsqr", chi2, "<=", dsqr, inputs=True):
        return [chi2, A.k(1.0)]
    s = A.sqrt(chi2)
    return [(A.k(2.0) * s) * delta - dsqr, A.div(delta, s)]


def _sim3_abc(A, sigma, s, theta, small, sn, cs, sigma_is_input):
    """A, B, C of sim3.h:92-133 (the constructor) and :169-212 (log): the four (sigma, theta) branches"""
    one = A.k(1.0)
    if A.cmp("|sigma|<1e-5", abs(sigma), "<", A.k(0.00001), inputs=sigma_is_input):
        C = one
        if small:
            a, b = A.k(1. / 2.), A.k(1. / 6.)
        else:
            theta2 = theta * theta
            a = A.div(one - cs, theta2)
            b = A.div(theta - sn, theta2 * theta)
    else:
        C = A.div(s - one, sigma)
        sigma2 = sigma * sigma
        if small:
            a = A.div((sigma - one) * s + one, sigma2)
            b = A.div(((A.k(0.5) * sigma2 - sigma) + one) * s, sigma2 * sigma)
        else:
            p, q = s * sn, s * cs
            theta2 = theta * theta
            c = theta2 + sigma2
            a = A.div(p * sigma + (one - q) * theta, theta * c)
            b = A.div((C - A.div((q - one) * sigma + p * theta, c)) * one, theta2)
    return a, b, C


def g_sim3_exp(A, u):
    """Sim3(const Vector7d&) (sim3.h:70-142)"""
    ox, oy, oz, sigma = u[0], u[1], u[2], u[6]
    theta = A.sqrt((ox * ox + oy * oy) + oz * oz)
    O = _skew(A, ox, oy, oz)
    s = A.fn("exp", sigma)
    O2, I = _mm(O, O), _eye(A)
    small = A.cmp("theta<1e-5", theta, "<", A.k(0.00001))
    sn, cs = A.k(0.0), A.k(1.0)
    if not small:
        sn, cs = A.fn("sin", theta), A.fn("cos", theta)
    a_, b_, c_ = _sim3_abc(A, sigma, s, theta, small, sn, cs, True)
    if small:
        R = [[(I[i][j] + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
    else:
        a, b = A.div(sn, theta), A.div(A.k(1.0) - cs, theta * theta)
        R = [[(I[i][j] + a * O[i][j]) + b * O2[i][j] for j in range(3)] for i in range(3)]
    q = g_qom(A, R)
    W = [[(a_ * O[i][j] + b_ * O2[i][j]) + c_ * I[i][j] for j in range(3)] for i in range(3)]
    return q + _mv(W, u[3:6]) + [s]


def g_sim3_mul(A, a, b):
    ax, ay, az, aw = a[0:4]
    bx, by, bz, bw = b[0:4]
    q = [((aw * bx + ax * bw) + ay * bz) - az * by, ((aw * by + ay * bw) + az * bx) - ax * bz,
         ((aw * bz + az * bw) + ax * by) - ay * bx, ((aw * bw - ax * bx) - ay * by) - az * bz]
    r = g_rotate(A, a[0:4], b[4:7])
    return q + [a[7] * r[i] + a[4 + i] for i in range(3)] + [a[7] * b[7]]


def g_sim3_inverse(A, S):
    qc = [-S[0], -S[1], -S[2], S[3]]
    f = A.div(A.k(-1.0), S[7])
    return qc + g_rotate(A, qc, [f * S[4], f * S[5], f * S[6]]) + [A.div(A.k(1.0), S[7])]


def g_lu3(A, W, t, inputs=False):
    """W.lu().solve(t): Eigen's PartialPivLU of a 3x3 as essential_graph_device.h states it"""
    W = [list(r) for r in W]
    perm = [0, 1, 2]
    for k in range(3):
        p, big = k, abs(W[k][k])
        for i in range(k + 1, 3):
            if A.cmp("pivot", abs(W[i][k]), ">", big, inputs=inputs and k == 0):
                big, p = abs(W[i][k]), i
        if p != k:
            W[k], W[p] = W[p], W[k]
            perm[k], perm[p] = perm[p], perm[k]
        if big != 0:
            for i in range(k + 1, 3):
                W[i][k] = A.div(W[i][k], W[k][k])
        for i in range(k + 1, 3):
            for j in range(k + 1, 3):
                W[i][j] = W[i][j] - W[i][k] * W[k][j]
    y = [t[perm[0]], t[perm[1]], t[perm[2]]]
    x = [None] * 3
    y[1] = y[1] - W[1][0] * y[0]
    y[2] = y[2] - W[2][0] * y[0]
    y[2] = y[2] - W[2][1] * y[1]
    x[2] = A.div(y[2], W[2][2])
    y[0] = y[0] - W[0][2] * x[2]
    y[1] = y[1] - W[1][2] * x[2]
    x[1] = A.div(y[1], W[1][1])
    y[0] = y[0] - W[0][1] * x[1]
    x[0] = A.div(y[0], W[0][0])
    return x


def g_sim3_log(A, S):
    """Sim3::log (sim3.h:148-230) -> omega, upsilon, sigma"""
    qx, qy, qz, qw = S[0:4]
    s, one, two = S[7], A.k(1.0), A.k(2.0)
    sigma = A.fn("log", s)
    tx, ty, tz = two * qx, two * qy, two * qz
    twx, twy, twz, txx, txy, txz = tx * qw, ty * qw, tz * qw, tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    R = [[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]]
    d = A.k(0.5) * (((R[0][0] + R[1][1]) + R[2][2]) - one)
    dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    small = A.cmp("d>1-eps", d, ">", A.k(1 - 0.00001))
    f, theta = A.k(0.5), A.k(0.0)
    sn, cs = A.k(0.0), A.k(1.0)
    if not small:
        theta = A.fn("acos", d)
        f = A.div(theta, two * A.sqrt(one - d * d))
        sn, cs = A.fn("sin", theta), A.fn("cos", theta)
    ox, oy, oz = f * dR[0], f * dR[1], f * dR[2]
    a_, b_, c_ = _sim3_abc(A, sigma, s, theta, small, sn, cs, False)
    O, I = _skew(A, ox, oy, oz), _eye(A)
    W = [[(a_ * O[i][j] + (((b_ * O[i][0]) * O[0][j] + (b_ * O[i][1]) * O[1][j]) + (b_ * O[i][2]) * O[2][j])) + c_ * I[i][j]
          for j in range(3)] for i in range(3)]
    return [ox, oy, oz] + g_lu3(A, W, S[4:7]) + [sigma]


def _jacobi_polar(A, T):
    """U V^T by the one-sided Jacobi essential_graph4_device.h states (float arithmetics only); untraced: the exact value is svd_r's"""
    k = A.k
    eps, tiny = (np.finfo(A.T).eps, np.finfo(A.T).tiny)
    G, V = [list(r) for r in T], _eye(A)
    dot = lambda X, i, j: (X[0][i] * X[0][j] + X[1][i] * X[1][j]) + X[2][i] * X[2][j]   # noqa: E731
    for _ in range(30):
        finished = True
        for i in range(2):
            for j in range(i + 1, 3):
                alpha, beta, gamma = dot(G, i, i), dot(G, j, j), dot(G, i, j)
                thr = (k(2.0) * eps) * A.sqrt(alpha * beta)
                if not (abs(gamma) > (thr if thr > tiny else tiny)):
                    continue
                finished = False
                tau = A.div(beta - alpha, k(2.0) * gamma)
                w = A.sqrt(tau * tau + k(1.0))
                t = A.div(k(1.0), tau + w) if tau >= 0 else A.div(k(1.0), tau - w)
                c = A.div(k(1.0), A.sqrt(t * t + k(1.0)))
                s = t * c
                for r in range(3):
                    gi, gj, vi, vj = G[r][i], G[r][j], V[r][i], V[r][j]
                    G[r][i], G[r][j] = c * gi - s * gj, s * gi + c * gj
                    V[r][i], V[r][j] = c * vi - s * vj, s * vi + c * vj
        if finished:
            break
    for j in range(3):
        n = A.sqrt(dot(G, j, j))
        for r in range(3):
            G[r][j] = A.div(G[r][j], n)
    return [[(G[r][0] * V[c][0] + G[r][1] * V[c][1]) + G[r][2] * V[c][2] for c in range(3)] for r in range(3)]


def g_polar(A, T):
    """NormalizeRotation (G2oTypes.h:68-71, ImuTypes.cc:34-37) and MLPnP's U V^T (:589-590): the orthogonal polar factor"""
    if A.kind == "mp":
        U, _, Vt = mp.svd_r(mp.matrix(T))
        M = U * Vt
        return [[M[i, j] for j in range(3)] for i in range(3)]
    if A.ortho == "jacobi":
        return _jacobi_polar(A, T)
    M = ic.normalize_rotation(np.array(T, A.T), A.ortho)
    assert M.dtype == A.T
    return [[M[i, j] for j in range(3)] for i in range(3)]


def g_exp_so3(A, x, y, z):
    """ExpSO3 (G2oTypes.cc:782-798)"""
    d2 = (x * x + y * y) + z * z
    d = A.sqrt(d2)
    W, I = _skew(A, x, y, z), _eye(A)
    if A.cmp("d<1e-5", d, "<", A.k(1e-5)):
        hW = [[A.k(0.5) * W[i][j] for j in range(3)] for i in range(3)]
        WW = _mm(hW, W)
        res = [[(I[i][j] + W[i][j]) + WW[i][j] for j in range(3)] for i in range(3)]
    else:
        WW = _mm(W, W)
        sn, cm = A.fn("sin", d), A.k(1.0) - A.fn("cos", d)
        res = [[(I[i][j] + A.div(W[i][j] * sn, d)) + A.div(WW[i][j] * cm, d2) for j in range(3)] for i in range(3)]
    return g_polar(A, res)


def g_log_so3(A, R):
    """LogSO3 (G2oTypes.cc:800-814): the early exits return the UNSCALED vector"""
    tr = (R[0][0] + R[1][1]) + R[2][2]
    two = A.k(2.0)
    w = [A.div(R[2][1] - R[1][2], two), A.div(R[0][2] - R[2][0], two), A.div(R[1][0] - R[0][1], two)]
    c = (tr - A.k(1.0)) * A.k(0.5)
    if A.cmp("cos>1", c, ">", A.k(1.0)) or A.cmp("cos<-1", c, "<", A.k(-1.0)):
        return w
    theta = A.fn("acos", c)
    s = A.fn("sin", theta)
    if A.cmp("|sin|<1e-5", abs(s), "<", A.k(1e-5)):
        return w
    return [A.div(theta * w[k], s) for k in range(3)]


def g_so3f_exp(A, w):
    """Sophus::SO3f::exp(w).matrix() (so3.hpp:583-619); the constants are the floats the reference's Scalar(...) makes"""
    k = lambda v: A.k(float(F32(v)))   # noqa: E731
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    if A.cmp("theta_sq<eps^2", th2, "<", A.k(float(F32(1e-5) * F32(1e-5)))):
        po4 = th2 * th2
        imag = (k(0.5) - k(1.0 / 48.0) * th2) + k(1.0 / 3840.0) * po4
        real = (k(1.0) - k(1.0 / 8.0) * th2) + k(1.0 / 384.0) * po4
    else:
        th = A.sqrt(th2)
        half = k(0.5) * th
        imag, real = A.div(A.fn("sin", half), th), A.fn("cos", half)
    x, y, z, qw = imag * w[0], imag * w[1], imag * w[2], real
    tx, ty, tz = k(2.0) * x, k(2.0) * y, k(2.0) * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * qw, ty * qw, tz * qw, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    one = k(1.0)
    return [[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]]


def g_bias_corrected(A, a):
    """GetDeltaRotation / Velocity / Position(b) and dbg of GetDeltaBias (ImuTypes.cc:277-308): float; a = the 80-double record"""
    dR, dV, dP = _m33(a[0:9]), a[9:12], a[12:15]
    JRg, JVg, JVa, JPg, JPa = (_m33(a[15 + 9 * i:24 + 9 * i]) for i in range(5))
    bias = a[60:66]
    dba = [A.narrow32(a[69 + k]) - bias[k] for k in range(3)]
    dbg = [A.narrow32(a[66 + k]) - bias[3 + k] for k in range(3)]
    N = g_polar(A, _mm(dR, g_so3f_exp(A, _mv(JRg, dbg))))
    p, q = _mv(JVg, dbg), _mv(JVa, dba)
    v = [(dV[k] + p[k]) + q[k] for k in range(3)]
    p, q = _mv(JPg, dbg), _mv(JPa, dba)
    return _flat(N) + v + [(dP[k] + p[k]) + q[k] for k in range(3)] + dbg


def g_right_jacobian(A, x, y, z):
    """RightJacobianSO3 (G2oTypes.cc:839-854)"""
    d2 = (x * x + y * y) + z * z
    d = A.sqrt(d2)
    W, I = _skew(A, x, y, z), _eye(A)
    if A.cmp("d<1e-5", d, "<", A.k(1e-5)):
        return I
    WW = _mm(W, W)
    a, b, c = A.k(1.0) - A.fn("cos", d), d - A.fn("sin", d), d2 * d
    return [[(I[i][j] - A.div(W[i][j] * a, d2)) + A.div(WW[i][j] * b, c) for j in range(3)] for i in range(3)]


def g_inverse_right_jacobian(A, x, y, z):
    """InverseRightJacobianSO3 (G2oTypes.cc:821-832)"""
    d2 = (x * x + y * y) + z * z
    d = A.sqrt(d2)
    W, I = _skew(A, x, y, z), _eye(A)
    if A.cmp("d<1e-5", d, "<", A.k(1e-5)):
        return I
    WW = _mm(W, W)
    one = A.k(1.0)
    k = A.div(one, d2) - A.div(one + A.fn("cos", d), (A.k(2.0) * d) * A.fn("sin", d))
    return [[(I[i][j] + A.div(W[i][j], A.k(2.0))) + WW[i][j] * k for j in range(3)] for i in range(3)]


DBL_EPS = 2.220446049250313e-16


def g_rodrigues2rot(A, w):
    """MLPnPsolver::rodrigues2rot (MLPnPsolver.cpp:703-718)"""
    R = _eye(A)
    th = A.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    if A.cmp("th>eps", th, ">", A.k(DBL_EPS)):
        K = _skew(A, w[0], w[1], w[2])
        a, b = A.div(A.fn("sin", th), th), A.div(A.k(1.0) - A.fn("cos", th), th * th)
        KK = _mm(K, K)
        R = [[(R[i][j] + a * K[i][j]) + b * KK[i][j] for j in range(3)] for i in range(3)]
    return R


def g_rot2rodrigues(A, R):
    """MLPnPsolver::rot2rodrigues (:720-735): acos of an argument above 1 is NaN, the comparison false, w = 0"""
    o = A.k(0.0)
    trace = ((R[0][0] + R[1][1]) + R[2][2]) - A.k(1.0)
    wnorm = A.fn("acos", A.div(trace, A.k(2.0)))
    if A.cmp("wnorm>eps", wnorm, ">", A.k(DBL_EPS)):
        sc = A.div(wnorm, A.k(2.0) * A.fn("sin", wnorm))
        return [(R[2][1] - R[1][2]) * sc, (R[0][2] - R[2][0]) * sc, (R[1][0] - R[0][1]) * sc]
    return [o, o, o]


def evaluate(fn, A, rec):
    """one record of `fn` in the arithmetic A -> the N_OUT[fn] outputs, in A's numbers.  Matrix and quaternion inputs of the
    direct tests are inputs=True: their comparisons are between inputs."""
    a = [A.k(x) for x in rec]
    if fn == "rotate":
        return g_rotate(A, a[0:4], a[4:7])
    if fn == "normalize_rotation":
        return g_normalize_q(A, a[0:4], inputs=True)
    if fn == "quaternion_of_matrix":
        return g_qom(A, _m33(a), inputs=True)
    if fn == "se3_exp":
        return g_se3_exp(A, a[0:6])
    if fn == "oplus":
        return g_oplus(A, a[0:7], a[7:13])
    if fn == "huber":
        return g_huber(A, a[0], a[1], rec[2] != 0)
    if fn == "sim3_exp":
        return g_sim3_exp(A, a[0:7])
    if fn == "sim3_mul":
        return g_sim3_mul(A, a[0:8], a[8:16])
    if fn == "sim3_inverse":
        return g_sim3_inverse(A, a[0:8])
    if fn == "lu3_solve":
        return g_lu3(A, _m33(a), a[9:12], inputs=True)
    if fn == "sim3_log":
        return g_sim3_log(A, a[0:8])
    if fn in ("normalize_rotation_eg4", "normalize_rotation_f", "mlpnp_nearest_rotation"):
        return _flat(g_polar(A, _m33(a)))
    if fn == "exp_so3":
        return _flat(g_exp_so3(A, a[0], a[1], a[2]))
    if fn == "log_so3":
        return g_log_so3(A, _m33(a))
    if fn == "so3f_exp_matrix":
        return _flat(g_so3f_exp(A, a[0:3]))
    if fn == "bias_corrected":
        return g_bias_corrected(A, a)
    if fn == "right_jacobian_so3":
        return _flat(g_right_jacobian(A, a[0], a[1], a[2]))
    if fn == "inverse_right_jacobian_so3":
        return _flat(g_inverse_right_jacobian(A, a[0], a[1], a[2]))
    if fn == "mlpnp_rodrigues2rot":
        return _flat(g_rodrigues2rot(A, a[0:3]))
    if fn == "mlpnp_rot2rodrigues":
        return g_rot2rodrigues(A, _m33(a))
    raise ValueError(fn)


def float_kind(fn):
    return "f32" if fn in FLOAT_CHAIN else "f64"


def run_float(fn, rec, nudge=False, ortho="jacobi"):
    A = Arith(float_kind(fn), nudge, ortho)
    with np.errstate(all="ignore"):
        out = evaluate(fn, A, rec)
    return np.array([float(v) for v in out], F64), A.trace


# ------------------------------------------------------------------------------------------------------- imported restatements
def _imported(fn, rec, nudge, ortho):
    """the project's own restatement of `fn`, or None where it has none / none with this option"""
    r = np.asarray(rec, F64)
    if fn == "rotate" and not nudge:
        return pc.rotate([float(c) for c in r[0:4]], r[4:7])
    if fn == "normalize_rotation" and not nudge:
        return pc.normalize_rotation(r[0:4])
    if fn == "quaternion_of_matrix" and not nudge:
        return sc3.quaternion_of_matrix(r[0:9].reshape(3, 3).tolist())
    if fn == "se3_exp" and not nudge:
        q, t = pc.se3_exp([float(c) for c in r[0:6]])
        return list(q) + list(t)
    if fn == "oplus" and not nudge:
        q, t = pc.oplus([float(c) for c in r[0:4]], [float(c) for c in r[4:7]], [float(c) for c in r[7:13]])
        return list(q) + list(t)
    if fn == "sim3_exp":
        q, t, s = sc3.sim3_exp([float(c) for c in r[0:7]], nudge)
        return list(q) + list(t) + [s]
    if fn in ("sim3_mul", "sim3_inverse") and not nudge:
        S = lambda v: ([float(c) for c in v[0:4]], [float(c) for c in v[4:7]], float(v[7]))   # noqa: E731
        q, t, s = sc3.sim3_mul(S(r[0:8]), S(r[8:16])) if fn == "sim3_mul" else sc3.sim3_inverse(S(r[0:8]))
        return list(q) + list(t) + [s]
    if fn == "exp_so3" and ortho != "jacobi":
        return ic.exp_so3(float(r[0]), float(r[1]), float(r[2]), nudge, ortho).ravel()
    if fn == "log_so3":
        return ic.log_so3(r[0:9].reshape(1, 3, 3), nudge)[0]
    if fn == "right_jacobian_so3":
        return ic.right_jacobian(r[None, 0:3], nudge).ravel()
    if fn == "inverse_right_jacobian_so3":
        return ic.inverse_right_jacobian(r[None, 0:3], nudge).ravel()
    if fn == "so3f_exp_matrix":
        return ic.so3f_exp(r[None, 0:3].astype(F32), nudge).ravel().astype(F64)
    if fn in ("normalize_rotation_eg4", "mlpnp_nearest_rotation") and ortho != "jacobi" and not nudge:
        return ic.normalize_rotation(r[0:9].reshape(3, 3).copy(), ortho).ravel()
    if fn == "normalize_rotation_f" and ortho != "jacobi" and not nudge:
        return ic.normalize_rotation(r[0:9].reshape(3, 3).astype(F32), ortho).ravel().astype(F64)
    return None


USES_POLAR = ("normalize_rotation_eg4", "normalize_rotation_f", "mlpnp_nearest_rotation", "exp_so3", "bias_corrected")


def variants(fn, rec):
    """every float restatement of one record: [(label, outputs float64 [N_OUT])]"""
    out = []
    orthos = ("jacobi", "svd", "polar") if fn in USES_POLAR else ("jacobi",)
    with np.errstate(all="ignore"):
        for nudge in (False, True):
            for ortho in orthos:
                out.append((f"own nudge={nudge} ortho={ortho}", run_float(fn, rec, nudge, ortho)[0]))
                v = _imported(fn, rec, nudge, ortho)
                if v is not None:
                    out.append((f"imported nudge={nudge} ortho={ortho}", np.array([float(c) for c in v], F64)))
    return out


# ------------------------------------------------------------------------------------------------------------------ records
PI = math.pi
_LO, _HI = float(np.nextafter(1e-5, 0.0)), float(np.nextafter(1e-5, 1.0))
NORMS = (0.0, 1e-200, 1e-9, _LO, 1e-5, _HI, 1e-4, 1e-2, 1.0, PI / 2, 2 * PI / 3, PI - 1e-8, PI, PI + 1e-8, 2 * PI - 1e-6, 2 * PI + 1e-6,
         10.0, 300.0, 1e6)
THRESHOLD_NORMS = (_LO, 1e-5, _HI)
TRANSLATIONS = ((0.0, 0.0, 0.0), (1.0, -2.0, 3.0), (1e3, 1e-3, -1.0))


def _directions():
    rng = np.random.default_rng(20241)
    axes = [(s * (k == 0), s * (k == 1), s * (k == 2)) for k in range(3) for s in (1.0, -1.0)]
    r3 = 1.0 / math.sqrt(3.0)
    diag = [(r3, r3, r3), (r3, r3, -r3), (r3, -r3, r3), (-r3, r3, r3)]
    rnd = rng.normal(size=(8, 3))
    rnd /= np.linalg.norm(rnd, axis=1)[:, None]
    return [("axis", a) for a in axes] + [("diag", d) for d in diag] + [("rand", tuple(float(c) for c in r)) for r in rnd]


DIRECTIONS = _directions()


_NAMES = {_LO: "below_1e-5", 1e-5: "1e-5", _HI: "above_1e-5", PI / 2: "pi/2", 2 * PI / 3: "2pi/3", 2 * PI / 3 - 1e-9: "2pi/3-1e-9",
          2 * PI / 3 + 1e-9: "2pi/3+1e-9", PI - 1e-8: "pi-1e-8", PI: "pi", PI + 1e-8: "pi+1e-8", PI - 1e-4: "pi-1e-4", PI + 1e-4: "pi+1e-4",
          2 * PI - 1e-6: "2pi-1e-6", 2 * PI + 1e-6: "2pi+1e-6"}


def norm_family(n):
    """one family per norm (so that an ill-conditioned norm widens no other norm's bound), named region:norm"""
    region = "small" if n < 1e-5 else ("just_above" if n <= 1e-4 else ("moderate" if n <= 2.2 else ("near_pi" if abs(n - PI) < 1e-3 else (
        "near_2pi" if abs(n - 2 * PI) < 1e-3 else "large"))))
    return region + ":" + _NAMES.get(n, f"{n:.3g}")


def rotation_vectors(qom=False, norms=None, extra_norms=()):
    """[(family, decided, (x, y, z))].  The threshold norms lie on the coordinate axes only, where sqrt(z*z) == |z| exactly decides the
    branch in every arithmetic (decided = True).  qom: the function converts its R to a quaternion (se3_exp, sim3_exp, oplus): a
    body diagonal ties the diagonal of R, so it is taken only where the trace branch is taken (cos(norm) > -0.25), and the double
    nearest pi, where the sign of the quaternion's w is the sign of sin(pi) ~ 1.2e-16 against the rounding of R, only on the axes,
    where R[1][0] - R[0][1] = 2 (sin / theta) z holds exactly (decided)."""
    out = []
    norms = tuple(NORMS if norms is None else norms) + tuple(extra_norms)
    if qom:   # at 2 pi / 3 the trace IS 0 up to rounding: its two neighbours, where the trace is -+ 1.7e-9, stand for it
        norms = tuple(m for n in norms for m in ((n - 1e-9, n + 1e-9) if n == 2 * PI / 3 else (n,)))
    for n in norms:
        for kind, d in DIRECTIONS:
            if (n in THRESHOLD_NORMS or n in extra_norms) and kind != "axis":
                continue
            if qom and kind == "diag" and not math.cos(n) > -0.25:
                continue
            if qom and n == PI and kind != "axis":
                continue
            # on an axis two diagonal entries of R are the same expression: the largest-diagonal comparison ties in every arithmetic
            decided = kind == "axis" and (n in THRESHOLD_NORMS or n in extra_norms or qom)
            out.append((norm_family(n), decided, tuple(n * c for c in d)))
    return out


def _rodrigues(axis, angle):
    """a rotation matrix in float64 (as orthonormal as float64 makes it)"""
    x, y, z = axis
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def _quat(axis, angle):
    s = math.sin(angle / 2)
    return np.array([axis[0] * s, axis[1] * s, axis[2] * s, math.cos(angle / 2)])


ANGLES = tuple(n for n in NORMS if 0 < n <= 10.0 and n != 1e-200)


def _half_turn(n):
    n = np.array(n, F64)
    return 2.0 * np.outer(n, n) - np.eye(3)


def edge_matrices(body_diagonals):
    """exact matrices: the identity, the three half turns about the axes, half turns about face diagonals (entries 0 and +-1) and,
    for quaternion_of_matrix, about the body diagonals, built so that the three tied diagonal entries are the same double (their
    trace is -1 only up to an ulp, which is on the exits of LogSO3 and rot2rodrigues)"""
    out = [np.eye(3), np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])]
    out += [np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, -1]]), np.array([[0.0, 0, 1], [0, -1, 0], [1, 0, 0]]), np.array([[-1.0, 0, 0], [0, 0, 1], [0, 1, 0]]),
            np.array([[0.0, -1, 0], [-1, 0, 0], [0, 0, -1]])]
    t, m = 2.0 / 3.0, 2.0 / 3.0 - 1.0
    for sx, sy, sz in ((1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1)) if body_diagonals else ():
        out.append(np.array([[m, sx * sy * t, sx * sz * t], [sx * sy * t, m, sy * sz * t], [sx * sz * t, sy * sz * t, m]]))
    return out


NEAR_PI_WIDE = (PI - 1e-4, PI + 1e-4)


def rotation_matrices(near_pi=None, qom=False):
    """[(family, decided, R [3, 3])] for the functions that read a rotation matrix.  near_pi: the angles beside pi, for the functions
    whose cosine, 1e-16 from -1 at pi +- 1e-8, would be on either side of -1 by the rounding of the matrix alone.  A matrix whose
    diagonal is exactly 1 (angles up to 1e-8) has an exact trace of 3: decided."""
    out = [("edge", True, R) for R in edge_matrices(qom)]
    angles = tuple(a for a in ANGLES if not (qom and a == 2 * PI / 3)) if near_pi is None else tuple(a for a in ANGLES if abs(a - PI) > 1e-3) + tuple(near_pi)
    for a in angles:
        for kind, d in DIRECTIONS:
            if a in THRESHOLD_NORMS and kind != "axis":
                continue
            R = _rodrigues(d, a)
            out.append((norm_family(a), bool(np.all(np.diag(R) == 1.0)), R))
    for kind, d in DIRECTIONS:                                   # trace just either side of 0
        for da in (-1e-9, 1e-9):
            out.append(("trace_switch", False, _rodrigues(d, 2 * PI / 3 + da)))
    return out


def _records(fn, rows):
    """rows: [(family, decided, values)] -> (records [n, in_width], families [n], decided [n])"""
    rec = np.zeros((len(rows), in_width(fn)), F64)
    for i, (_, _, v) in enumerate(rows):
        v = np.asarray(v, F64).ravel()
        rec[i, :len(v)] = v
    return rec, [r[0] for r in rows], np.array([bool(r[1]) for r in rows])


def _f32(v):
    return np.asarray(v, F64).astype(F32).astype(F64)


def _build(fn):
    rng = np.random.default_rng(OPS.index(fn) + 977)
    rows = []
    if fn in ("exp_so3", "right_jacobian_so3", "inverse_right_jacobian_so3"):
        rows = rotation_vectors()
    elif fn == "mlpnp_rodrigues2rot":
        e = DBL_EPS
        rows = rotation_vectors(extra_norms=(float(np.nextafter(e, 0.0)), e, float(np.nextafter(e, 1.0))))
    elif fn == "se3_exp":
        rows = [(f, d, w + t) for f, d, w in rotation_vectors(qom=True) for t in TRANSLATIONS]
    elif fn == "oplus":
        poses = [np.r_[_quat(DIRECTIONS[6 + 3 * k][1], a), t] for k, (a, t) in enumerate(zip((0.3, 2.5, PI - 1e-3), TRANSLATIONS))]
        rows = [(f, d, np.r_[poses[i % 3], w, TRANSLATIONS[(i + 1) % 3]]) for i, (f, d, w) in enumerate(rotation_vectors(qom=True))]
    elif fn == "sim3_exp":
        sig = (0.0, 1e-6, -1e-6, _LO, -_LO, 1e-5, -1e-5, 0.05, -0.05, 1.0, -1.0, 5.0)
        sub = rotation_vectors(qom=True, norms=(0.0, 1e-9, _LO, 1e-5, _HI, 1e-2, 1.0, PI - 1e-8, 2 * PI + 1e-6, 300.0))
        for i, (f, d, w) in enumerate(sub):
            for j, s in enumerate(sig):
                # sigma is an input: |sigma| < 1e-5 is decided exactly, whatever the record
                rows.append((f + ("_sigma0" if abs(s) < 1e-5 else "_sigma"), d, w + TRANSLATIONS[(i + j) % 3] + (s,)))
    elif fn == "so3f_exp_matrix":
        root = float(np.sqrt(F32(1e-5) * F32(1e-5)))
        f = lambda v, k: float(F32(v) if k == 0 else (np.nextafter(F32(v), F32(1)) if k > 0 else np.nextafter(F32(v), F32(0))))   # noqa: E731
        # two ulps either side of the root: theta_sq moves one ulp per ulp of z, past the half ulp its rounding can move it
        norms = (0.0, 1e-30, 1e-9, f(f(root, -1), -1), f(f(root, 1), 1), 1e-4, 1e-2, 1.0, PI / 2, 2 * PI / 3, PI - 1e-4, PI, PI + 1e-4,
                 2 * PI - 1e-3, 2 * PI + 1e-3, 10.0, 300.0)
        for n in norms:
            n = float(F32(n))
            thr = abs(n - root) < 1e-9
            for kind, d in DIRECTIONS:
                if thr and kind != "axis":
                    continue
                fam = ("small" if n < root else ("just_above" if n <= 1e-3 else ("moderate" if n < 2.2 else "large"))) + f":{n:.9g}"
                rows.append((fam, thr, _f32(np.array(d) * n)))
    elif fn in ("quaternion_of_matrix", "log_so3", "mlpnp_rot2rodrigues"):
        rows = rotation_matrices(None, True) if fn == "quaternion_of_matrix" else rotation_matrices(NEAR_PI_WIDE)
        if fn != "quaternion_of_matrix":
            # costheta above 1 and below -1 (acos gets an argument outside [-1, 1]): one diagonal entry moved by 2^-50, one ulp of the
            # trace, so that the float sum is exact and the exit is decided in exact arithmetic
            up, dn = np.eye(3), np.diag([-1.0, -1.0, 1.0])
            up[0, 0] = 1.0 + 2.0 ** -50
            dn[0, 0] = -1.0 - 2.0 ** -50
            rows += [("edge", True, up), ("edge", True, dn)]
            # angles either side of |sin theta| = 1e-5, at both ends
            for a in (1e-5 - 1e-8, 1e-5 + 1e-8, PI - 1e-5 - 1e-8, PI - 1e-5 + 1e-8):
                rows += [("sin_exit", False, _rodrigues(d, a)) for _, d in DIRECTIONS[:6] + DIRECTIONS[10:13]]
    elif fn == "rotate":
        for a in ANGLES + (0.0,):
            for k, (_, d) in enumerate(DIRECTIONS):
                rows.append(("all", False, np.r_[_quat(d, a), TRANSLATIONS[(k + 1) % 3] if k % 3 else rng.normal(size=3)]))
    elif fn == "normalize_rotation":
        for a in ANGLES + (0.0,):
            for k, (kind, d) in enumerate(DIRECTIONS):
                q = _quat(d, a) * (1.0, 1 + 1e-7, 3.0, -0.5)[k % 4]
                rows.append(("all", False, q))
        rows += [("all", True, q) for q in ([1.0, 0, 0, 0], [0, 2.0, 0, 0.0], [0, 0, -1.0, -0.0], [0.5, 0.5, 0.5, 0.5], [0.6, 0, 0.8, -0.0])]
    elif fn in ("sim3_mul", "sim3_inverse"):
        scales = (1.0, 1 + 1e-6, 1 - 1e-6, 0.5, 20.0)
        for i, a in enumerate(ANGLES + (0.0,)):
            for k, (_, d) in enumerate(DIRECTIONS):
                A_ = np.r_[_quat(d, a), TRANSLATIONS[k % 3], scales[(i + k) % 5]]
                B_ = np.r_[_quat(DIRECTIONS[(k + 5) % 18][1], ANGLES[(i + 3) % len(ANGLES)]), TRANSLATIONS[(k + 1) % 3], scales[(i + 2 * k) % 5]]
                rows.append(("all", False, np.r_[A_, B_]))
    elif fn == "sim3_log":
        e = math.exp(1e-5)
        scales = (1.0, 1 + 1e-6, 1 - 1e-6, float(np.nextafter(e, 0.0)), float(np.nextafter(e, 2.0)), float(np.nextafter(1 / e, 0.0)),
                  float(np.nextafter(1 / e, 2.0)), math.exp(1e-5 * (1 - 1e-6)), math.exp(-1e-5 * (1 + 1e-6)), 0.5, 20.0)
        quats = [("edge", np.array(q)) for q in ([0, 0, 0, 1.0], [1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0])]
        for a in tuple(a for a in ANGLES if abs(a - PI) > 1e-3) + NEAR_PI_WIDE:   # as rotation_matrices(NEAR_PI_WIDE)
            if a in THRESHOLD_NORMS:
                continue
            # a quarter turn about a coordinate axis makes W(1,1) = W(2,1) = 1 / theta: a true tie of the LU's pivot search, which
            # rounding decides.  Taken about the other directions only.
            quats += [(norm_family(a), _quat(d, a)) for kind, d in DIRECTIONS[::2] if not (a == PI / 2 and kind == "axis") and not (a == 2 * PI / 3 and kind == "diag")]   # (the same for a third of a turn about a body diagonal)
        # d = cos(angle) either side of 1 - 1e-5
        quats += [("cos_switch", _quat(d, a)) for a in (math.sqrt(2e-5) * (1 - 1e-6), math.sqrt(2e-5) * (1 + 1e-6)) for _, d in DIRECTIONS[::3]]
        for i, (f, q) in enumerate(quats):
            for j in range(3):
                s = scales[(3 * i + j) % len(scales)] if f != "edge" else scales[j]
                rows.append((f, False, np.r_[q, TRANSLATIONS[(i + j) % 3], s]))
    elif fn in ("normalize_rotation_eg4", "normalize_rotation_f", "mlpnp_nearest_rotation"):
        base = [_rodrigues(d, a) for a in (1e-4, 1.0, 2 * PI / 3, PI - 1e-8, 10.0) for _, d in DIRECTIONS[::4]] + [np.eye(3)]
        for R in base:
            S3, S8 = np.eye(3), np.eye(3)
            S3[0, 1], S8[1, 2] = 1e-3, 1e-8
            rows += [("scaled", False, R * (1 + 1e-7)), ("shear_1e-3", False, R @ S3), ("shear_1e-8", False, R @ S8),
                     ("columns", False, R * np.array([1.0, 2.0, 0.5])[None, :]), ("orthonormal", False, R)]
        rows.append(("reflection", False, base[3] @ np.diag([1.0, 1.0, -1.0])))
        if fn == "normalize_rotation_f":   # (a shear of 1e-8 is below the float's ulp: those records are the rotation as float makes it)
            rows = [(f, d, _f32(R)) for f, d, R in rows]
    elif fn == "lu3_solve":
        M = lambda *r: np.array(r, F64)   # noqa: E731
        t = (1.0, -2.0, 3.0)
        named = [("no_pivot", False, M([4, 1, 2], [1, 3, 0.5], [2, 0.5, 5])), ("pivot_col0", False, M([1, 1, 2], [4, 3, 0.5], [2, 0.5, 5])),
                 ("pivot_col1", False, M([4, 1, 2], [1, 0.5, 0.5], [2, 3, 5])), ("pivot_both", False, M([1, 2, 3], [2, 4.5, 1], [4, 1, 2])),
                 ("tie", True, M([2, 1, 0], [-2, 3, 1], [2, 0, 4])), ("tie", True, M([4, 1, 2], [2, 1.5, 1], [2, 1.5, 5])),
                 ("singular", True, M([0, 1, 2], [0, 3, 1], [0, 2, 4]))]
        rows = [(f, d, np.r_[W.ravel(), t]) for f, d, W in named]
        for _ in range(200):
            W = rng.normal(size=(3, 3)) + 2 * np.eye(3)
            if np.linalg.cond(W) < 50:
                rows.append(("random", False, np.r_[W.ravel(), rng.normal(size=3)]))
    elif fn == "huber":
        for delta in (1.0, math.sqrt(5.991), math.sqrt(7.815)):
            d2 = delta * delta
            for chi2 in (0.0, float(np.nextafter(d2, 0.0)), d2, float(np.nextafter(d2, math.inf)), 1e300, 0.5 * d2, 9.0 * d2):
                for robust in (0.0, 1.0):
                    rows.append(("all", False, (chi2, delta, robust)))
    elif fn == "bias_corrected":
        for i in range(60):
            dR = np.asarray(_rodrigues(DIRECTIONS[i % 18][1], (0.0, 1e-3, 0.3, 2.0)[i % 4]), F64).astype(F32)
            bias = rng.normal(size=6) * (0.1, 0.1, 0.1, 0.01, 0.01, 0.01)
            delta = (0.0, 1e-7, 1e-3, 0.1)[(i // 4) % 4]
            if i < 40:
                fam, J = "scaled", [rng.normal(size=(3, 3)) * s for s in (0.5, 0.3, 0.3, 0.1, 0.1)]
            else:   # |JRg dbg| = s 1e-3 sqrt(3) either side of the float threshold 1e-5
                delta = 1e-3
                s = (5e-3, 7e-3)[i % 2]
                fam, J = ("below_threshold", "above_threshold")[i % 2], [np.eye(3) * s] + [rng.normal(size=(3, 3)) * 0.2 for _ in range(4)]
            b32 = _f32(bias)
            g = b32[3:6] + delta * np.array([1.0, 1.0, -1.0])
            a_ = b32[0:3] + delta * np.array([-1.0, 2.0, 0.5])
            if delta == 0.0:
                fam = "zero_delta"
            v = np.concatenate([_f32(dR).ravel(), _f32(rng.normal(size=3)), _f32(rng.normal(size=3) * 0.3)] + [_f32(j).ravel() for j in J] + [b32, g, a_])
            rows.append((fam, False, v))
    else:
        raise ValueError(fn)
    return _records(fn, rows)


@functools.lru_cache(maxsize=None)
def records(fn):
    return _build(fn)


# --------------------------------------------------------------------------------------------------------- exact and distance
@functools.lru_cache(maxsize=None)
def exact(fn):
    """-> (values: per record a list of mpf, traces, margins)"""
    rec, _, _ = records(fn)
    vals, traces, margins = [], [], []
    for r in rec:
        A = EXACT()
        vals.append(evaluate(fn, A, r))
        traces.append(A.trace)
        margins.append(A.margins)
    return vals, traces, margins


def distance(out, ex):
    """max |difference| / max(1, max |exact|) over the finite positions of the exact value; None if a non-finite position of the
    exact value is not the same class in `out`"""
    fin = [e for e in ex if mp.isfinite(e)]
    scale = max([mp.mpf(1)] + [abs(e) for e in fin])
    d = mp.mpf(0)
    for o, e in zip(out, ex):
        o = float(o)
        if mp.isnan(e):
            if not math.isnan(o):
                return None
        elif mp.isinf(e):
            if not (math.isinf(o) and (o > 0) == (e > 0)):
                return None
        else:
            if not math.isfinite(o):
                return None
            d = max(d, abs(mp.mpf(o) - e))
    return float(d / scale)


def distances(fn, outputs):
    """outputs [n, >= N_OUT] -> per record distance to the exact value (inf where the class of a non-finite position differs)"""
    ex = exact(fn)[0]
    k = N_OUT[fn]
    return np.array([math.inf if (d := distance(outputs[i][:k], ex[i])) is None else d for i in range(len(ex))])


def condition_violations(fn):
    """records that sit where the exact value and a float run could part: [(index, what)]"""
    rec, _, decided = records(fn)
    _, traces, margins = exact(fn)
    floor = MARGIN_MIN_F32 if fn in FLOAT_CHAIN else MARGIN_MIN
    bad = []
    for i, r in enumerate(rec):
        for nudge in (False, True):
            if run_float(fn, r, nudge)[1] != traces[i]:
                bad.append((i, f"the float run (nudge={nudge}) takes other branches: {traces[i]}"))
        if not decided[i]:
            bad += [(i, f"{tag}: margin {m:.3g}") for tag, m in margins[i] if m < floor]
    return bad


@functools.lru_cache(maxsize=None)
def measure(fn):
    """D(fn, family): the largest distance between the exact value and any variant over the family's records"""
    rec, fams, _ = records(fn)
    ex = exact(fn)[0]
    D = {}
    for i, r in enumerate(rec):
        for label, v in variants(fn, r):
            d = distance(v, ex[i])
            assert d is not None, (fn, i, label, v, ex[i])
            D[fams[i]] = max(D.get(fams[i], 0.0), d)
    return D


def measure_all():
    return {fn: measure(fn) for fn in OPS}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def judge(fn, out, host=None):
    """out [n, LIE_OUT]: what the host program (host=None) or the device (host = the host program's output) returned for records(fn).
    The host program is held to 16 D on every family; the device to byte-equality with the host program on the families bits_bound
    names and to 16 D on the others; non-finite positions of the exact value to the same class; unused outputs to 0.
    -> (largest distance / D over the families with D > 0, the same over the records not byte-equal to `host`, their number,
    failures)"""
    rec, fams, _ = records(fn)
    D = golden()[fn]
    out = np.asarray(out, F64)
    assert out.shape == (len(rec), LIE_OUT), out.shape
    dist = distances(fn, out)
    worst, worst_differing, failures = 0.0, 0.0, []
    differ = 0 if host is None else int(np.sum(np.any(out.view(np.uint64) != np.asarray(host, F64).view(np.uint64), axis=1)))
    for i, d in enumerate(dist):
        Df = D[fams[i]]
        if np.any(out[i, N_OUT[fn]:].view(np.uint64) != 0):
            failures.append((i, fams[i], "an unused output is not +0"))
        if math.isinf(d):
            failures.append((i, fams[i], "a non-finite position of the exact value is another class", out[i, :N_OUT[fn]].tolist()))
            continue
        if Df > 0:
            worst = max(worst, d / Df)
            if host is not None and out[i].tobytes() != np.asarray(host[i], F64).tobytes():
                worst_differing = max(worst_differing, d / Df)
        if host is not None and bits_bound(fn, fams[i], Df):
            if out[i].tobytes() != np.asarray(host[i], F64).tobytes():
                failures.append((i, fams[i], "not byte-equal to the host program", out[i, :N_OUT[fn]].tolist(), host[i][:N_OUT[fn]].tolist()))
        elif not d <= MARGIN * Df:
            failures.append((i, fams[i], f"distance {d:.3g} > 16 D = {MARGIN * Df:.3g}", rec[i][:9].tolist()))
    return worst, worst_differing, differ, failures


def statement_mismatches(fn, out):
    """records of the bits_bound families where the host program differs from a float restatement of the same statement (the headers'
    Jacobi, no nudge): [(index, family, label)]"""
    rec, fams, _ = records(fn)
    D = golden()[fn]
    bad = []
    for i, r in enumerate(rec):
        if not bits_bound(fn, fams[i], D[fams[i]]):
            continue
        for label, v in variants(fn, r):
            if "nudge=False ortho=jacobi" in label and v.tobytes() != np.asarray(out[i][:N_OUT[fn]], F64).tobytes():
                bad.append((i, fams[i], label))
    return bad


# ------------------------------------------------------------------------------------ files of tests/lie_probe_main.cc
def write_blocks(path, blocks):
    """blocks: [(fn, records [n, in_width])]"""
    with open(path, "wb") as f:
        f.write(struct.pack("=i", len(blocks)))
        for fn, rec in blocks:
            rec = np.ascontiguousarray(rec, F64).reshape(-1, in_width(fn))
            f.write(struct.pack("=ii", OPS.index(fn), len(rec)))
            f.write(rec.tobytes())


def read_blocks(path, blocks):
    raw = np.fromfile(path, F64)
    out, at = [], 0
    for fn, rec in blocks:
        n = len(np.asarray(rec).reshape(-1, in_width(fn)))
        out.append(raw[at:at + n * LIE_OUT].reshape(n, LIE_OUT).copy())
        at += n * LIE_OUT
    assert at == len(raw), (at, len(raw))
    return out


if __name__ == "__main__":
    if sys.argv[1:] == ["--write-golden"]:
        M = measure_all()
        with open(GOLDEN, "w") as f:
            json.dump(M, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", GOLDEN)
    for fn in OPS:
        bad = condition_violations(fn)
        print(fn, len(records(fn)[0]), "records", {k: f"{v:.3g}" for k, v in measure(fn).items()}, "violations:", len(bad))
        for i, what in bad[:8]:
            print("   ", i, records(fn)[1][i], what, records(fn)[0][i][:9])
