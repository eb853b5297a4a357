"""The small dense decompositions one at a time (msorb_debug_decomp, ms-slam_amd/csrc/decomp_probe_device.h): the records of every
op by named family, built from fixed seeds; float restatements of each routine, statement by statement, that also keep a trace
(sweeps, rotations, the arms of the 2x2 step, swaps, negations, refusals of the floor test); the measures each output is judged by,
which do not depend on which of several valid answers a routine picks; D(op, family, measure), the largest value of the measure that
an independent computation in the same precision (numpy's LAPACK on the float32 array for float ops, on float64 for double ops)
reaches on the family's records, floored at n eps; and the files of tests/decomp_probe_main.cc.  DESIGN.md section 23.

    python tests/decomp_cases.py --write-golden     rewrites tests/golden/decomp_sensitivity.json
"""
import functools
import itertools
import json
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "decomp_sensitivity.json")
F32, F64, LD = np.float32, np.float64, np.longdouble
EPS32, EPS64 = float(np.finfo(F32).eps), float(np.finfo(F64).eps)
FLT_MIN, FLT_MAX = F32(1.17549435e-38), F32(3.402823466e+38)
K_BORDER_MAX = 9                                   # kBorderMax
DECOMP_OUT = 24
OPS = ("tv_inverse3", "tv_det3", "tv_svd3", "tv_null_vector_8", "tv_null_vector_16", "np_null_vector", "sim3_largest_eigenvector",
       "sim3_rotation_of_quaternion", "mlpnp_rank3", "mlpnp_eig3", "mlpnp_solve6", "mlpnp_null_vector_12", "mlpnp_null_vector_9",
       "inertial_ldlt")
IN_WIDTH = dict(zip(OPS, (9, 9, 9, 72, 144, 16, 16, 4, 9, 9, 42, 144, 81, 1 + K_BORDER_MAX * K_BORDER_MAX + K_BORDER_MAX)))
FLOAT_OPS = OPS[:8]
COOPERATIVE = {"tv_null_vector_8": 9, "tv_null_vector_16": 9, "mlpnp_null_vector_12": 12, "mlpnp_null_vector_9": 12}   # the mismatch slot
SWEEP_CAP = {"tv_svd3": 30, "tv_null_vector_8": 30, "tv_null_vector_16": 30, "np_null_vector": 60, "sim3_largest_eigenvector": 16,
             "mlpnp_eig3": 30, "mlpnp_null_vector_12": 30, "mlpnp_null_vector_9": 30}
DIM = {"tv_inverse3": 3, "tv_det3": 3, "tv_svd3": 3, "tv_null_vector_8": 9, "tv_null_vector_16": 9, "np_null_vector": 4,
       "sim3_largest_eigenvector": 4, "sim3_rotation_of_quaternion": 4, "mlpnp_rank3": 3, "mlpnp_eig3": 3, "mlpnp_solve6": 6,
       "mlpnp_null_vector_12": 12, "mlpnp_null_vector_9": 9, "inertial_ldlt": K_BORDER_MAX}
FACTOR = 16.0                                      # one more ordering of the same arithmetic
# tv_null_vector's rotation test is the documented relative one while the largest column norm N of the matrix it is given lies in
# [2^-12, 2^30] (two_view_device.h); below, down to about 1e-19, the threshold degrades to FLT_MIN; beyond either end nothing rotates
TV_DOMAIN = (2.0 ** -12, 2.0 ** 30)


def in_width(op):
    return IN_WIDTH[op]


def eps_of(op):
    return EPS32 if op in FLOAT_OPS else EPS64


def _mx(a, b):
    """np_max: b > a ? b : a (a NaN b is ignored, a NaN a is replaced)"""
    return b if b > a else a


# ------------------------------------------------------------------------------------------------------------ restatements
# Each returns the routine's output and fills `tr`, a dict of counters.  Scalars are numpy scalars of the routine's type: every
# operation is one correctly rounded IEEE operation, as the np_* operators are.

def _count(tr, key, n=1):
    tr[key] = tr.get(key, 0) + n


def two_sided_jacobi(A, n, tr, svd3):
    """tv_svd3 (n = 3, svd3 = True) -> (U, S, V), or np_null_vector (n = 4, svd3 = False) -> x; float32"""
    f = F32
    A = np.asarray(A, f).reshape(n, n)
    tiny, precision = FLT_MIN, f(2.384185791015625e-07)
    scale = f(0)
    for e in np.abs(A).reshape(-1):
        scale = _mx(scale, e)
    if svd3:
        if not scale > 0 or not scale <= FLT_MAX:
            scale = f(1)
    elif scale == 0:
        scale = f(1)
    W = (A / scale).astype(f)
    U, V = np.eye(n, dtype=f), np.eye(n, dtype=f)
    max_diag = f(0)
    if svd3:
        max_diag = _mx(_mx(abs(W[0, 0]), abs(W[1, 1])), abs(W[2, 2]))
    else:
        max_diag = _mx(_mx(abs(W[0, 0]), abs(W[1, 1])), _mx(abs(W[2, 2]), abs(W[3, 3])))
    for sweep in range(30 if svd3 else 60):
        finished = True
        for p in range(1, n):
            for q in range(p):
                thr = _mx(tiny, precision * max_diag)
                if not (abs(W[p, q]) > thr or abs(W[q, p]) > thr):
                    continue
                finished = False
                _count(tr, "rotations")
                m00, m01, m10, m11 = W[p, p], W[p, q], W[q, p], W[q, q]
                t, d = m00 + m11, m10 - m01
                c1, s1 = f(1), f(0)
                if not abs(d) < tiny:
                    u = t / d
                    tmp = np.sqrt(f(1) + u * u)
                    s1, c1 = f(1) / tmp, u / tmp
                else:
                    _count(tr, "|d|<tiny")
                n00, n01, n11 = c1 * m00 + s1 * m10, c1 * m01 + s1 * m11, c1 * m11 - s1 * m01
                cr, sr = f(1), f(0)
                deno = f(2) * abs(n01)
                if not deno < tiny:
                    tau = (n00 - n11) / deno
                    w = np.sqrt(tau * tau + f(1))
                    _count(tr, "tau>0" if tau > 0 else "tau<0" if tau < 0 else "tau==0")
                    tt = f(1) / (tau + w) if tau > 0 else f(1) / (tau - w)
                    nn = f(1) / np.sqrt(tt * tt + f(1))
                    mag = abs(tt) * nn
                    sr = -mag if (tt > 0) == (n01 > 0) else mag
                    cr = nn
                else:
                    _count(tr, "deno<tiny")
                cl, sl = c1 * cr + s1 * sr, s1 * cr - c1 * sr
                a, b = W[p].copy(), W[q].copy()
                W[p], W[q] = cl * a + sl * b, cl * b - sl * a
                if svd3:
                    ua, ub = U[:, p].copy(), U[:, q].copy()
                    U[:, p], U[:, q] = cl * ua + sl * ub, cl * ub - sl * ua
                a, b = W[:, p].copy(), W[:, q].copy()
                W[:, p], W[:, q] = cr * a - sr * b, sr * a + cr * b
                va, vb = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = cr * va - sr * vb, sr * va + cr * vb
                max_diag = _mx(max_diag, _mx(abs(W[p, p]), abs(W[q, q])))
        if finished:
            break
        _count(tr, "sweeps")
    if svd3:
        sv = np.zeros(3, f)
        for i in range(3):
            a = W[i, i]
            sv[i] = abs(a)
            if a < 0:
                U[:, i] = -U[:, i]
                _count(tr, "negated")
        sv = (sv * scale).astype(f)
        for i in range(2):
            pos = i
            best = sv[i]
            for k in range(i + 1, 3):
                if sv[k] > best:
                    best, pos = sv[k], k
            if pos != i:
                _count(tr, f"swap{i}")
                sv[[i, pos]] = sv[[pos, i]]
                U[:, [i, pos]] = U[:, [pos, i]]
                V[:, [i, pos]] = V[:, [pos, i]]
        return U, sv, V
    sv = [abs(W[i, i]) for i in range(4)]
    col = [0, 1, 2, 3]
    stop = False
    for i in range(4):
        pos = i
        best = sv[i]
        for k in range(i + 1, 4):
            if sv[k] > best:
                best, pos = sv[k], k
        if best == 0:
            stop = True
            _count(tr, "zero maximum")
        if not stop and pos != i:
            _count(tr, f"swap{i}")
            sv[i], sv[pos] = sv[pos], sv[i]
            col[i], col[pos] = col[pos], col[i]
    return V[:, col[3]].copy()


def _sum_rows(P):
    """the sums over the rows in ascending order, one rounding per addition (np.cumsum adds left to right)"""
    return np.cumsum(P, axis=0, dtype=P.dtype)[-1]


def one_sided_jacobi(A, tr):
    """tv_null_vector on A [rows, 9] float32 -> x [9]"""
    f = F32
    A = np.array(A, f)
    tiny, precision, floor_rel = FLT_MIN, f(2.384185791015625e-07), f(3.63797880709171295e-12)
    V = np.eye(9, dtype=f)
    max_norm = f(0)
    for s in _sum_rows(A * A):
        max_norm = _mx(max_norm, s)
    floor2 = floor_rel * max_norm
    for sweep in range(30):
        finished = True
        for p in range(8):
            for q in range(p + 1, 9):
                a, b = A[:, p], A[:, q]
                alpha, beta, gamma = _sum_rows(np.stack([a * a, b * b, a * b], 1))
                thr = _mx(tiny, precision * np.sqrt(alpha * beta))
                if not abs(gamma) > thr:
                    continue
                if not alpha > floor2 or not beta > floor2:
                    _count(tr, "floor refused")
                    continue
                finished = False
                _count(tr, "rotations")
                tau = (beta - alpha) / (f(2) * gamma)
                _count(tr, "tau>0" if tau > 0 else "tau<0" if tau < 0 else "tau==0")
                ww = np.sqrt(tau * tau + f(1))
                t = f(1) / (tau + ww) if tau >= 0 else f(1) / (tau - ww)
                c = f(1) / np.sqrt(t * t + f(1))
                s = t * c
                for M in (A, V):
                    a, b = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = c * a - s * b, s * a + c * b
        if finished:
            break
        _count(tr, "sweeps")
    best, least = 0, f(0)
    for c, s in enumerate(_sum_rows(A * A)):
        if c == 0 or s < least:
            least, best = s, c
        elif s == least:
            _count(tr, "minimum tie")
    return V[:, best].copy()


def symmetric_jacobi(A, n, max_sweeps, tr):
    """the cyclic Jacobi of sim3_largest_eigenvector (float32, n = 4), mlpnp_eig3 (float64, n = 3) and mlpnp_null_vector
    (float64, n = 12 or 9) in A's type -> (diagonal, V)"""
    f = A.dtype.type
    tiny = FLT_MIN if f is F32 else f(2.2250738585072014e-308)
    precision = f(2) * f(EPS32 if f is F32 else EPS64)
    W = np.array(A, f).reshape(n, n)
    V = np.eye(n, dtype=f)
    max_diag = abs(W[0, 0])
    for i in range(1, n):
        max_diag = _mx(max_diag, abs(W[i, i]))
    for sweep in range(max_sweeps):
        finished = True
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = W[p, q]
                thr = _mx(tiny, precision * max_diag)
                if not abs(apq) > thr:
                    continue
                finished = False
                _count(tr, "rotations")
                app, aqq = W[p, p], W[q, q]
                tau = (aqq - app) / (f(2) * apq)
                _count(tr, "tau>0" if tau > 0 else "tau<0" if tau < 0 else "tau==0")
                w = np.sqrt(tau * tau + f(1))
                t = f(1) / (tau + w) if tau >= 0 else f(1) / (tau - w)
                c = f(1) / np.sqrt(t * t + f(1))
                s = t * c
                kp, kq = W[:, p].copy(), W[:, q].copy()
                nkp, nkq = c * kp - s * kq, s * kp + c * kq
                W[:, p] = nkp
                W[p, :] = nkp
                W[:, q] = nkq
                W[q, :] = nkq
                W[p, p], W[q, q] = app - t * apq, aqq + t * apq
                W[p, q] = W[q, p] = 0
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
                max_diag = _mx(_mx(max_diag, abs(W[p, p])), abs(W[q, q]))
        if finished:
            break
        _count(tr, "sweeps")
    return np.diag(W).copy(), V


def largest_eigenvector(A, tr):
    d, V = symmetric_jacobi(np.asarray(A, F32), 4, 16, tr)
    best = 0
    for i in range(1, 4):
        if d[i] > d[best]:
            best = i
        elif d[i] == d[best]:
            _count(tr, "maximum tie")
    return V[:, best].copy()


def eig3(M, tr):
    d, V = symmetric_jacobi(np.asarray(M, F64), 3, 30, tr)
    used, E = [False] * 3, np.zeros((3, 3))
    for k in range(3):
        best = -1
        for i in range(3):
            if not used[i] and (best < 0 or d[i] < d[best]):
                best = i
        used[best] = True
        E[k] = V[:, best]
    return E


def smallest_vector(Wm, nc, tr):
    d, V = symmetric_jacobi(np.asarray(Wm, F64), nc, 30, tr)
    col = 0
    for i in range(1, nc):
        if abs(d[i]) < abs(d[col]):
            col = i
        elif abs(d[i]) == abs(d[col]):
            _count(tr, "minimum tie")
    x = np.zeros(12)
    x[:nc] = V[:, col]
    return x


def rank3(M, tr):
    """mlpnp_rank3"""
    f = F64
    prec = f(EPS64) * f(3.0)
    tiny = f(2.2250738585072014e-308)
    a = np.array(M, f).reshape(3, 3)
    piv = [f(0)] * 3
    biggest = maxpivot = f(0)
    nonzero = 3
    with np.errstate(all="ignore"):
        for k in range(3):
            big, pr, pc = abs(a[k, k]), k, k
            for c in range(k, 3):
                for r in range(k, 3):
                    if abs(a[r, c]) > big:
                        big, pr, pc = abs(a[r, c]), r, c
            if k == 0:
                biggest = big
            if big <= biggest * prec:
                nonzero = k
                _count(tr, f"nonzero={k}")
                if big == biggest * prec:
                    _count(tr, "big==bound")
                break
            a[[k, pr], :] = a[[pr, k], :]
            a[:, [k, pc]] = a[:, [pc, k]]
            c0 = a[k, k]
            tailsq = f(0)
            for i in range(k + 1, 3):
                tailsq = a[i, k] * a[i, k] if i == k + 1 else tailsq + a[i, k] * a[i, k]
            ess, tau, beta = [f(0)] * 3, f(0), c0
            if not tailsq <= tiny:
                beta = np.sqrt(c0 * c0 + tailsq)
                if c0 >= 0:
                    beta = -beta
                for i in range(k + 1, 3):
                    ess[i] = a[i, k] / (c0 - beta)
                tau = (beta - c0) / beta
            elif k < 2:
                _count(tr, "tailsq<=tiny")
            piv[k] = beta
            if abs(beta) > maxpivot:
                maxpivot = abs(beta)
            for j in range(k + 1, 3):
                tmp = f(0)
                for i in range(k + 1, 3):
                    tmp = ess[i] * a[i, j] if i == k + 1 else tmp + ess[i] * a[i, j]
                tmp = tmp + a[k, j]
                a[k, j] = a[k, j] - tau * tmp
                for i in range(k + 1, 3):
                    a[i, j] = a[i, j] - (tau * ess[i]) * tmp
        return sum(1 for i in range(nonzero) if abs(piv[i]) > maxpivot * prec)


def det3(M):
    M = np.asarray(M, F32).reshape(-1)

    def term(a, b, c):
        return M[a] * (M[3 + b] * M[6 + c] - M[3 + c] * M[6 + b])
    return (term(0, 1, 2) - term(1, 0, 2)) + term(2, 0, 1)


def inverse3(M):
    M = np.asarray(M, F32).reshape(-1)
    cof = np.zeros(9, F32)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            cof[3 * i + j] = M[3 * i1 + j1] * M[3 * i2 + j2] - M[3 * i1 + j2] * M[3 * i2 + j1]
    det = (M[0] * cof[0] + M[1] * cof[1]) + M[2] * cof[2]
    invdet = F32(1) / det
    return (cof.reshape(3, 3).T * invdet).astype(F32).reshape(-1)


def rotation_of_quaternion(q):
    f = F32
    q = np.asarray(q, f)
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    w, x, y, z = (q[i] / n for i in range(4))
    tx, ty, tz = f(2) * x, f(2) * y, f(2) * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    one = f(1)
    return np.array([one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
                     one - (txx + tyy)], f)


def solve6(S, g):
    S = np.asarray(S, F64).reshape(6, 6)
    L, D, y, dx = np.zeros((6, 6)), np.zeros(6), np.zeros(6), np.zeros(6)
    for j in range(6):
        d = S[j, j]
        for k in range(j):
            d = d - (L[j, k] * L[j, k]) * D[k]
        D[j] = d
        for i in range(j + 1, 6):
            v = S[i, j]
            for k in range(j):
                v = v - (L[i, k] * L[j, k]) * D[k]
            L[i, j] = v / d
    for i in range(6):
        v = g[i]
        for k in range(i):
            v = v - L[i, k] * y[k]
        y[i] = v
    for i in range(5, -1, -1):
        v = y[i] / D[i]
        for k in range(i + 1, 6):
            v = v - L[k, i] * dx[k]
        dx[i] = v
    return dx


def ldlt(n, A, b, tr):
    """ldlt_factor on the upper triangle of A [n, n], then ldlt_apply -> (ok, x [n]); x stays 0 on a refusal"""
    A = np.asarray(A, F64).reshape(n, n)
    Lf, rinv, x, y = np.zeros((n, n)), np.zeros(n), np.zeros(n), np.zeros(n)
    for j in range(n):
        v = np.zeros(n)
        d = A[j, j]
        for m in range(j):
            v[m] = Lf[j, m] * Lf[m, m]
            d = d - Lf[j, m] * v[m]
        if not d > 0:
            _count(tr, f"refused at {j}")
            return 0.0, x
        Lf[j, j] = d
        rinv[j] = F64(1.0) / d
        for i in range(j + 1, n):
            s = A[j, i]
            for m in range(j):
                s = s - Lf[i, m] * v[m]
            Lf[i, j] = s * rinv[j]
    for i in range(n):
        s = b[i]
        for m in range(i):
            s = s - Lf[i, m] * y[m]
        y[i] = s
    for i in range(n - 1, -1, -1):
        s = y[i] * rinv[i]
        for m in range(i + 1, n):
            s = s - Lf[m, i] * x[m]
        x[i] = s
    return 1.0, x


def restated(op, rec):
    """(the 24 outputs of one record as the restatement gives them, its trace)"""
    tr, o = {}, np.zeros(DECOMP_OUT)
    with np.errstate(all="ignore"):
        if op == "tv_inverse3":
            o[:9] = inverse3(rec)
        elif op == "tv_det3":
            o[0] = det3(rec)
        elif op == "tv_svd3":
            U, S, V = two_sided_jacobi(rec, 3, tr, True)
            o[:9], o[9:12], o[12:21] = U.reshape(-1), S, V.reshape(-1)
        elif op in ("tv_null_vector_8", "tv_null_vector_16"):
            o[:9] = one_sided_jacobi(np.asarray(rec, F32).reshape(-1, 9), tr)
        elif op == "np_null_vector":
            o[:4] = two_sided_jacobi(rec, 4, tr, False)
        elif op == "sim3_largest_eigenvector":
            o[:4] = largest_eigenvector(np.asarray(rec, F32), tr)
        elif op == "sim3_rotation_of_quaternion":
            o[:9] = rotation_of_quaternion(rec)
        elif op == "mlpnp_rank3":
            o[0] = rank3(rec, tr)
        elif op == "mlpnp_eig3":
            o[:9] = eig3(rec, tr).reshape(-1)
        elif op == "mlpnp_solve6":
            o[:6] = solve6(rec[:36], rec[36:42])
        elif op in ("mlpnp_null_vector_12", "mlpnp_null_vector_9"):
            nc = 12 if op.endswith("12") else 9
            o[:12] = smallest_vector(np.asarray(rec, F64), nc, tr)
        elif op == "inertial_ldlt":
            n = int(rec[0]) if 1 <= rec[0] <= K_BORDER_MAX and rec[0] == int(rec[0]) else 0
            if n == 0:
                o[0] = -1.0                                                  # the probe's own guard: nothing is called
            else:
                o[0], o[1:1 + n] = ldlt(n, rec[1:1 + n * n], rec[1 + n * n:1 + n * n + n], tr)
    return o, tr


@functools.lru_cache(maxsize=None)
def restated_all(op):
    rec = records(op)[0]
    outs, traces = zip(*(restated(op, r) for r in rec))
    return np.array(outs), list(traces)


# ------------------------------------------------------------------------------------------------------------------ records
def _rng(op, fam):
    return np.random.RandomState(zlib.crc32(f"{op}/{fam}".encode()))


def _orth(rng, n):
    Q, R = np.linalg.qr(rng.standard_normal((n, n)))
    return Q * np.sign(np.diag(R))


def _spec(rng, m, n, s):
    """U diag(s) V^T, U [m, len(s)] and V [n, len(s)] with orthonormal columns"""
    s = np.asarray(s, F64)
    return (_orth(rng, m)[:, :len(s)] * s) @ _orth(rng, n)[:, :len(s)].T


def _sym(rng, n, lam):
    Q = _orth(rng, n)
    A = (Q * np.asarray(lam, F64)) @ Q.T
    return (A + A.T) / 2


def _r32(A):
    with np.errstate(over="ignore"):
        return np.asarray(A, F64).astype(F32).astype(F64)


def _unit_max(A):
    return A / np.abs(A).max()


class _Records:
    def __init__(self, op):
        self.op, self.rec, self.fam = op, [], []

    def add(self, fam, A):
        """one record: A flattened, rounded to float for a float op, padded with zeros to the op's width"""
        a = np.asarray(A, F64).reshape(-1)
        if self.op in FLOAT_OPS:
            a = _r32(a)
        r = np.zeros(IN_WIDTH[self.op])
        r[:len(a)] = a
        self.rec.append(r)
        self.fam.append(fam)

    def rng(self, fam):
        return _rng(self.op, fam)


PERMS3 = list(itertools.permutations(range(3)))


def _perm(p, scales):
    P = np.zeros((len(p), len(p)))
    for i, j in enumerate(p):
        P[i, j] = scales[i]
    return P


def _non_finite(B, base, symmetric=False, at=1, n=None):
    base = np.array(base, F64)
    for fam, v in (("one NaN", np.nan), ("one +inf", np.inf)):
        A = base.copy()
        A.reshape(-1)[at] = v
        if symmetric:
            A[at % n, at // n] = v
        B.add("non-finite: " + fam, A)
    B.add("non-finite: all inf", np.full_like(base, np.inf))


def _square_float(B, n):
    """the families shared by the square float SVD ops: tv_svd3 (n = 3) and np_null_vector (n = 4)"""
    e = EPS32
    sep = [1.0, 0.6, 0.25] if n == 3 else [1.0, 0.8, 0.6, 0.3]
    grd = [1.0, 1e-3, 1e-6] if n == 3 else [1.0, 1e-2, 1e-4, 1e-6]
    r = B.rng("generic")
    for _ in range(8):
        B.add("generic", r.standard_normal((n, n)))
    r = B.rng("separated")
    for _ in range(6):
        B.add("separated", _spec(r, n, n, sep) * r.uniform(0.5, 2.0))
    r = B.rng("graded")
    for _ in range(4):
        B.add("graded", _spec(r, n, n, grd))
    r = B.rng("repeated")
    for _ in range(3):
        B.add("repeated", _orth(r, n))                                   # a rotation or reflection: all equal
    for _ in range(3):
        B.add("repeated", _spec(r, n, n, [1.0, 1.0] + [0.0] * (n - 2)))   # the essential-matrix shape
    for _ in range(2):
        B.add("repeated", 2.5 * _orth(r, n))
    if n == 4:
        for _ in range(2):
            B.add("repeated", _spec(r, 4, 4, [1.0, 1.0, 0.5, 0.5]))
    r = B.rng("clustered")
    for _ in range(4):
        B.add("clustered", _spec(r, n, n, [1.0 - 3 * e * k for k in range(n)]))
    for rank in range(n - 1, 0, -1):
        r = B.rng(f"rank {rank}")
        for _ in range(3 if n == 3 else 4):
            B.add(f"rank {rank}", _spec(r, n, n, sep[:rank]))
    B.add("identity", np.eye(n))
    B.add("identity", -np.eye(n))
    scales = [1.0, 2.0, 3.0, 4.0][:n]
    perms = PERMS3 if n == 3 else [(3, 2, 1, 0), (1, 0, 3, 2), (2, 3, 0, 1), (0, 1, 2, 3), (1, 2, 3, 0), (3, 0, 1, 2), (0, 2, 1, 3), (2, 0, 3, 1)]
    for p in perms:                                                       # the reordering swaps: all six orders for the 3x3
        B.add("permutation", _perm(p, scales))
        B.add("permutation", _perm(p, [-s if i % 2 == 0 else s for i, s in enumerate(scales)]))
    for d in ([-1.0, 3.0, -2.0, 0.5], [2.0, -5.0, 0.5, -5.0], [0.0, -1.0, 4.0, 4.0]):
        B.add("diagonal", np.diag(d[:n]))
    r = B.rng("skew")
    for _ in range(3):
        S = r.standard_normal((n, n))
        B.add("skew", _r32(S) - _r32(S).T)
    r = B.rng("zero column")
    for c in (0, n - 1):
        A = r.standard_normal((n, n))
        A[:, c] = 0
        B.add("zero column", A)
    r = B.rng("equal columns")
    for c in ((0, 1), (0, n - 1)):
        A = _r32(r.standard_normal((n, n)))
        A[:, c[1]] = A[:, c[0]]
        B.add("equal columns", A)
    B.add("zero", np.zeros((n, n)))
    H = np.array([[1.0, 1, 0], [1, -1, 0], [0, 0, 2]]) if n == 3 else np.array([[1.0, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]])
    B.add("orthogonal columns", H)
    B.add("orthogonal columns", H * np.array([4.0, 0.5, 1.0, 2.0][:n]))
    r = B.rng("scale")
    G = [_r32(_unit_max(r.standard_normal((n, n)))) for _ in range(2)]
    for A in G:
        for k in (-120, -90, -60, -30, 30, 60, 90, 120):
            B.add("scale", A * 2.0 ** k)
        for k in (-128, -138, -146):
            B.add("scale: denormal", A * 2.0 ** k)
        # the largest entry FLT_MAX for the null vector; for the SVD, whose S must hold sigma_1, sigma_1 = 0.99 FLT_MAX
        B.add("scale: near FLT_MAX", A * float(FLT_MAX) * (0.99 / np.linalg.svd(A, compute_uv=False)[0] if n == 3 else 1.0))
        B.add("scale: near FLT_MAX", A * 2.0 ** 126)
    _non_finite(B, G[0])


def _tv3(B):
    """tv_inverse3 and tv_det3"""
    r = B.rng("generic")
    for _ in range(12):
        B.add("generic", r.standard_normal((3, 3)))
    r = B.rng("conditioned")
    for k in range(7):
        for _ in range(2):
            B.add("conditioned", _spec(r, 3, 3, [1.0, 10.0 ** (-k / 2), 10.0 ** -k]))
    r = B.rng("rotation")
    for _ in range(3):
        B.add("rotation", _orth(r, 3))
    for p in PERMS3:
        B.add("permutation", _perm(p, [2.0, -0.5, 3.0]))
    for d in ([-1.0, 3.0, -2.0], [2.0, -5.0, 0.5], [1.0, 1.0, 1.0]):
        B.add("diagonal", np.diag(d))
    B.add("singular", [[1, 2, 3], [4, 5, 6], [7, 8, 9]])
    B.add("singular", np.zeros((3, 3)))
    B.add("singular", [[1, 0, 2], [3, 0, 4], [5, 0, 6]])
    B.add("singular", [[1, 1, 2], [3, 3, 4], [5, 5, 6]])
    r = B.rng("nearly singular")
    for _ in range(4):
        B.add("nearly singular", _spec(r, 3, 3, [1.0, 0.5, 1e-6]))
    r = B.rng("scale")
    G = [_r32(_unit_max(r.standard_normal((3, 3)))) for _ in range(2)]
    for A in G:
        for k in (-20, -10, 10, 20):
            B.add("scale", A * 2.0 ** k)
    _non_finite(B, G[0])


def _hadamard(n):
    H = np.array([[1.0]])
    while len(H) < n:
        H = np.block([[H, H], [H, -H]])
    return H


def _design(r, rows):
    """a design matrix of ComputeF21 (8 rows) or ComputeH21 (16 rows) on eight pairs normalised to mean deviation 1"""
    p = r.standard_normal((8, 4))
    p = p - p.mean(0)
    p = _r32(p / np.abs(p).mean(0))
    A = np.zeros((rows, 9))
    for i, (u1, v1, u2, v2) in enumerate(p):
        if rows == 8:
            A[i] = [u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1]
        else:
            A[2 * i] = [0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2]
            A[2 * i + 1] = [u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2]
    return A


def _tv_null(B, rows):
    m = min(rows, 9)                                                        # the rank a rows x 9 matrix can have
    r = B.rng("generic")
    for _ in range(6):
        B.add("generic", r.standard_normal((rows, 9)))
    r = B.rng("design")
    for _ in range(4):
        B.add("design", _design(r, rows))
    r = B.rng("separated")
    sep = list(np.linspace(2.0, 1.3, 8)) + ([0.5] if rows == 16 else [])
    for _ in range(5):
        B.add("separated", _spec(r, rows, 9, sep))
    r = B.rng("graded")
    for _ in range(4):
        B.add("graded", _spec(r, rows, 9, np.logspace(0, -6, m)))
    for nullity in (1, 2, 4):
        r = B.rng(f"nullity {nullity}")
        for _ in range(4 if nullity < 4 else 3):
            B.add(f"nullity {nullity}", _spec(r, rows, 9, np.linspace(2.0, 1.0, 9 - nullity)))
    r = B.rng("repeated")
    for _ in range(3):
        B.add("repeated", _spec(r, rows, 9, np.ones(m)))
    r = B.rng("clustered")
    for _ in range(3):
        B.add("clustered", _spec(r, rows, 9, [1.0 - 3 * EPS32 * k for k in range(m)]))
    eye = np.zeros((rows, 9))
    eye[:m, :m] = np.eye(m)
    B.add("identity", eye)                                                  # (8 rows: the ninth column is zero)
    B.add("identity", -eye)
    r = B.rng("permutation")
    for _ in range(3):
        A = np.zeros((rows, 9))
        for c, row in enumerate(r.permutation(rows)[:m]):
            A[row, c] = 2.0 ** r.randint(-3, 4) * (1 if c % 2 else -1)
        B.add("permutation", A[:, r.permutation(9)])
    r = B.rng("zero column")
    for c in (0, 8):
        A = r.standard_normal((rows, 9))
        A[:, c] = 0
        B.add("zero column", A)
    r = B.rng("equal columns")
    for c in ((0, 1), (2, 8)):
        A = _r32(r.standard_normal((rows, 9)))
        A[:, c[1]] = A[:, c[0]]
        B.add("equal columns", A)
    r = B.rng("rank one")
    for _ in range(2):
        B.add("rank one", _spec(r, rows, 9, [1.0]))
    B.add("zero", np.zeros((rows, 9)))
    H = _hadamard(rows)[:, :9] if rows == 16 else np.hstack([_hadamard(8), np.zeros((8, 1))])
    B.add("orthogonal columns", H)                                          # zero rotations, every minimum a tie
    B.add("orthogonal columns", H[:, ::-1] * 0.25)
    r = B.rng("scale")
    G = [_r32(r.standard_normal((rows, 9))) for _ in range(2)]
    for A in G:
        for k in (-10, -6, 6, 12, 20, 26):
            B.add("scale", A * 2.0 ** k)
        for k in (-20, -40, -50):
            B.add("scale: below the domain", A * 2.0 ** k)
        for k in (-68, 50, 63):
            B.add("scale: nothing rotates", A * 2.0 ** k)
    _non_finite(B, G[0], at=10)
    A = G[0].copy()
    A[3, 0] = np.nan
    B.add("non-finite: one NaN", A)                                         # in the first column


def _sym_common(B, n, double, sep, grd):
    e = EPS64 if double else EPS32
    r = B.rng("generic")
    for _ in range(8):
        A = r.standard_normal((n, n))
        B.add("generic", (A + A.T) / 2)
    r = B.rng("separated")
    for _ in range(6):
        B.add("separated", _sym(r, n, sep))
    r = B.rng("graded")
    for _ in range(4):
        B.add("graded", _sym(r, n, grd))
    r = B.rng("clustered")
    for _ in range(4):
        B.add("clustered", _sym(r, n, [1.0 - 3 * e * k for k in range(n)]))
    B.add("identity", np.eye(n))
    B.add("identity", -np.eye(n))
    r = B.rng("rank one")
    for _ in range(3):
        B.add("rank one", _sym(r, n, [1.0] + [0.0] * (n - 1)))
    B.add("zero", np.zeros((n, n)))
    r = B.rng("zero diagonal")
    for _ in range(3):
        A = r.standard_normal((n, n))
        A = (A + A.T) / 2
        np.fill_diagonal(A, 0.0)
        B.add("zero diagonal", A)                                           # max_diag == 0 at entry


def _sim3_eig(B):
    _sym_common(B, 4, False, [1.0, 0.5, -0.2, -0.9], [1.0, 1e-2, 1e-4, 1e-6])
    r = B.rng("doubled largest")
    for _ in range(4):
        B.add("doubled largest", _sym(r, 4, [1.0, 1.0, 0.3, -0.5]))
    B.add("doubled largest", np.diag([2.0, 1.0, 2.0, -1.0]))                # the first maximum
    r = B.rng("all equal")
    for _ in range(2):
        B.add("all equal", _sym(r, 4, [1.5] * 4))
    r = B.rng("negative definite")
    for _ in range(4):
        B.add("negative definite", _sym(r, 4, [-0.1, -0.5, -1.0, -2.0]))
    r = B.rng("traceless")
    for _ in range(6):                                                       # Horn's N of a random M
        M = _r32(r.standard_normal((3, 3)))
        N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                      [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                      [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                      [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
        N = _r32(N)
        B.add("traceless", N + np.triu(N, 1).T)
    for d in ([-1.0, 3.0, -2.0, 0.5], [2.0, -5.0, 0.5, 2.0], [0.0, -1.0, 4.0, 4.0]):
        B.add("diagonal", np.diag(d))
    B.add("permutation", [[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 2], [0, 0, 2, 0]])
    B.add("permutation", [[0, 0, 0, 3], [0, 1, 0, 0], [0, 0, -1, 0], [3, 0, 0, 0]])
    r = B.rng("scale")
    for _ in range(2):
        A = r.standard_normal((4, 4))
        A = _r32(_unit_max((A + A.T) / 2))
        for k in (-100, -60, -30, 30, 60, 100):
            B.add("scale", A * 2.0 ** k)
    A = r.standard_normal((4, 4))
    _non_finite(B, (A + A.T) / 2, symmetric=True, n=4)


def _quaternion(B):
    r = B.rng("generic")
    for _ in range(16):
        B.add("generic", r.standard_normal(4))
    r = B.rng("unit")
    for _ in range(8):
        q = r.standard_normal(4)
        B.add("unit", q / np.linalg.norm(q))
    for i in range(4):
        for s in (1.0, -3.0):
            q = np.zeros(4)
            q[i] = s
            B.add("axis", q)
    r = B.rng("small w")
    for k in (-6, -12, -20, -30):
        q = r.standard_normal(4)
        q[0] *= 2.0 ** k
        B.add("small w", q)
    r = B.rng("scale")
    G = [_r32(r.standard_normal(4)) for _ in range(2)]
    for q in G:
        for k in (-60, -30, -10, 10, 30, 60):
            B.add("scale", q * 2.0 ** k)
    _non_finite(B, G[0])
    B.add("non-finite: zero", np.zeros(4))


def _rank3(B):
    B.add("integer: rank 0", np.zeros((3, 3)))
    for v in ([1, 0, 0], [0, 2, 0], [0, 0, 3], [0, -4, 0], [5, 0, 0]):        # one non-zero entry: every operation exact
        B.add("integer: rank 1", np.outer(v, v))
    r = B.rng("integer: rank 2")
    for axis in (0, 1, 2, 0, 1, 2, 0, 1):                                     # six integer points in a coordinate plane: P P^T
        P = r.randint(-4, 5, (3, 6)).astype(F64)
        P[axis] = 0
        B.add("integer: rank 2", P @ P.T)
    r = B.rng("integer: rank 3")
    for _ in range(8):
        A = r.randint(-2, 3, (3, 3)).astype(F64)
        B.add("integer: rank 3", A + A.T + 12 * np.eye(3))                    # diagonally dominant
    for p in PERMS3:
        B.add("permutation", _perm(p, [3.0, -1.0, 2.0]))
    r = B.rng("integer: coplanar")
    for nrm in ([1, 1, 1], [1, 2, -1], [2, -1, 3], [1, -1, 0], [3, 1, 1], [1, 0, 2]):   # a plane through the origin, not a coordinate plane
        nrm = np.array(nrm)
        b1 = [np.cross(nrm, e) for e in np.eye(3, dtype=int) if np.any(np.cross(nrm, e))][0]
        basis = [b1, np.cross(nrm, b1)]
        P = sum(np.outer(b, r.randint(-3, 4, 6)) for b in basis).astype(F64)
        B.add("integer: coplanar", P @ P.T)
    r = B.rng("clear gap: rank 3")
    for ratio in (1.0, 0.5, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 2e-8):           # sigma_3 / sigma_1
        B.add("clear gap: rank 3", _sym(r, 3, [1.0, np.sqrt(ratio), ratio]))
    r = B.rng("near the rule")
    for f in (0.3, 0.5, 0.8, 1.0, 1.25, 2.0, 3.0, 3.6):                       # sigma_3 / sigma_1 = f * 3 eps
        B.add("near the rule", _sym(r, 3, [1.0, 0.5, f * 3 * EPS64]))
    # the largest entry of the second corner EQUALS 3 eps times the first pivot's, exactly: the rule's `<=` ends the decomposition
    # there (rank 1); with `<` the corner's column, of norm sqrt(2) b, would pass the closing count as a second pivot
    b = 3 * EPS64
    for s in (1.0, 2.0 ** -40, 2.0 ** 200):
        B.add("on the rule", np.array([[1, 0, 0], [0, b, b], [0, b, b]]) * s)
    B.add("on the rule", np.array([[b, 0, -b], [0, 1, 0], [-b, 0, b]]))
    r = B.rng("scale")
    for k in (-300, -100, 100, 300):
        for ratio in (0.5, 1e-6):
            B.add("scale", _sym(r, 3, [1.0, np.sqrt(ratio), ratio]) * 2.0 ** k)
    A = r.standard_normal((3, 3))
    _non_finite(B, A + A.T, symmetric=True, n=3)


def _eig3(B):
    _sym_common(B, 3, True, [1.0, 0.4, -0.5], [1.0, 1e-6, 1e-12])
    r = B.rng("repeated")
    for lam in ([1.0, 1.0, 2.0], [1.0, 2.0, 2.0], [1.5, 1.5, 1.5]):
        for _ in range(2):
            B.add("repeated", _sym(r, 3, lam))
    r = B.rng("planar")
    for _ in range(4):                                                        # P P^T of six coplanar points: what the caller gives it
        P = _orth(r, 3)[:, :2] @ r.standard_normal((2, 6)) * 3
        B.add("planar", P @ P.T)
    for d in ([-1.0, 3.0, -2.0], [2.0, -5.0, 2.0], [0.0, 4.0, 4.0]):
        B.add("diagonal", np.diag(d))
    B.add("permutation", [[0, 1, 0], [1, 0, 0], [0, 0, 2]])
    B.add("permutation", [[0, 0, 3], [0, 1, 0], [3, 0, 0]])
    r = B.rng("scale")
    for _ in range(2):
        A = r.standard_normal((3, 3))
        A = _unit_max((A + A.T) / 2)
        for k in (-300, -150, -50, 50, 150, 300):
            B.add("scale", A * 2.0 ** k)
    A = r.standard_normal((3, 3))
    _non_finite(B, A + A.T, symmetric=True, n=3)


def _mlpnp_null(B, nc):
    sep = list(np.linspace(1.0, 0.3, nc - 1)) + [0.05]
    _sym_common(B, nc, True, sep, np.logspace(0, -12, nc))
    r = B.rng("gram")
    for _ in range(6):                                                        # A^T A of a 12-row design matrix
        A = r.standard_normal((12, nc))
        B.add("gram", A.T @ A)
    for nullity in (1, 2, 4):
        r = B.rng(f"nullity {nullity}")
        for _ in range(3):
            B.add(f"nullity {nullity}", _sym(r, nc, list(np.linspace(2.0, 1.0, nc - nullity)) + [0.0] * nullity))
    r = B.rng("repeated")
    for _ in range(3):
        B.add("repeated", _sym(r, nc, [1.5] * nc))
    r = B.rng("indefinite")
    for _ in range(3):
        B.add("indefinite", _sym(r, nc, [(-1.0) ** k * (0.2 + k) for k in range(nc)]))
    r = B.rng("diagonal")
    for _ in range(3):
        d = r.randint(-4, 5, nc).astype(F64)                                  # unsorted, negative, tied
        B.add("diagonal", np.diag(d))
    r = B.rng("permutation")
    for _ in range(2):
        p = r.permutation(nc)
        P = np.zeros((nc, nc))
        P[np.arange(nc), p] = 1
        B.add("permutation", (P + P.T) * 0.5 + np.diag(r.randint(0, 3, nc)))
    r = B.rng("zero column")
    for c in (0, nc - 1):
        A = r.standard_normal((12, nc))
        A[:, c] = 0
        B.add("zero column", A.T @ A)
    r = B.rng("equal columns")
    for c in ((0, 1), (2, nc - 1)):
        A = r.standard_normal((12, nc))
        A[:, c[1]] = A[:, c[0]]
        B.add("equal columns", A.T @ A)
    r = B.rng("scale")
    for _ in range(2):
        A = r.standard_normal((12, nc))
        A = _unit_max(A.T @ A)
        for k in (-300, -100, 100, 300):
            B.add("scale", A * 2.0 ** k)
    A = r.standard_normal((12, nc))
    _non_finite(B, A.T @ A, symmetric=True, n=nc)


def _ldl_integer(n, bad, value, r):
    """L D L^T with a unit lower L of small integers and D = 1 or 2 except D[bad] = value: an integer matrix whose pivots the
    factorisation computes exactly"""
    L = np.tril(r.randint(-2, 3, (n, n)).astype(F64), -1) + np.eye(n)
    D = r.randint(1, 3, n).astype(F64)
    if not np.isnan(value):
        D[bad] = value
    S = (L * D) @ L.T
    if np.isnan(value):
        S[bad, bad] = np.nan
    return S


def _spd(r, n, cond):
    return _sym(r, n, np.logspace(0, -np.log10(cond), n) if n > 1 else [1.0])


def _solve6(B):
    r = B.rng("conditioned")
    for k in range(13):
        for _ in range(2):
            B.add("conditioned", np.concatenate([_spd(r, 6, 10.0 ** k).reshape(-1), r.standard_normal(6)]))
    r = B.rng("gram")
    for _ in range(6):
        J = r.standard_normal((12, 6))
        B.add("gram", np.concatenate([(J.T @ J).reshape(-1), J.T @ r.standard_normal(12)]))
    for d in (np.ones(6), [2.0, 0.5, 4.0, 1.0, 8.0, 0.25], [3.0] * 6):
        B.add("diagonal", np.concatenate([np.diag(d).reshape(-1), np.arange(1.0, 7.0)]))
    r = B.rng("pivot")
    for col in (0, 3, 5):
        B.add("pivot: negative", np.concatenate([_ldl_integer(6, col, -2.0, r).reshape(-1), r.randint(-3, 4, 6)]))
        B.add("pivot: zero", np.concatenate([_ldl_integer(6, col, 0.0, r).reshape(-1), r.randint(1, 4, 6)]))
        B.add("pivot: NaN", np.concatenate([_ldl_integer(6, col, np.nan, r).reshape(-1), r.randint(-3, 4, 6)]))
    r = B.rng("scale")
    for _ in range(2):
        S, g = _spd(r, 6, 100.0), r.standard_normal(6)
        for k in (-400, -100, 100, 400):
            B.add("scale", np.concatenate([S.reshape(-1) * 2.0 ** k, g * 2.0 ** k]))
    S, g = _spd(r, 6, 10.0), r.standard_normal(6)
    for fam, v in (("one NaN", np.nan), ("one +inf", np.inf)):
        gg = g.copy()
        gg[2] = v
        B.add("non-finite: " + fam, np.concatenate([S.reshape(-1), gg]))
    B.add("non-finite: all inf", np.full(42, np.inf))


def _ldlt_record(n, A, b):
    return np.concatenate([[float(n)], np.asarray(A, F64).reshape(-1), np.asarray(b, F64).reshape(-1)])


def _ldlt(B):
    r = B.rng("conditioned")
    for n, ks in ((9, range(13)), (3, (0, 4, 8, 12)), (6, (0, 4, 8, 12))):
        for k in ks:
            B.add("conditioned", _ldlt_record(n, _spd(r, n, 10.0 ** k), r.standard_normal(n)))
    for a, b in ((2.0, 3.0), (1e300, 1.0), (1e-300, -1.0)):
        B.add("n = 1", _ldlt_record(1, [a], [b]))
    r = B.rng("gram")
    for n in (2, 4, 5, 7, 8, 9):
        J = r.standard_normal((n + 3, n))
        B.add("gram", _ldlt_record(n, J.T @ J, r.standard_normal(n)))
    r = B.rng("pivot")
    for n in (9, 3):
        for col in (0, n // 2, n - 1):
            for fam, v in (("zero", 0.0), ("negative", -2.0), ("NaN", np.nan)):
                B.add("pivot: " + fam, _ldlt_record(n, _ldl_integer(n, col, v, r), r.randint(-3, 4, n)))
    for fam, v in (("zero", 0.0), ("negative", -2.0), ("NaN", np.nan)):
        B.add("pivot: " + fam, _ldlt_record(1, [v], [1.0]))
    r = B.rng("lower triangle ignored")
    for n, junk in ((9, np.nan), (4, np.inf), (2, 1e300)):
        S = _spd(r, n, 100.0)
        S[np.tril_indices(n, -1)] = junk                                     # only the upper triangle is read
        B.add("lower triangle ignored", _ldlt_record(n, S, r.standard_normal(n)))
    r = B.rng("scale")
    for n in (9, 3):
        S, g = _spd(r, n, 100.0), r.standard_normal(n)
        for k in (-400, -100, 100, 400):
            B.add("scale", _ldlt_record(n, S * 2.0 ** k, g * 2.0 ** k))
    S, g = _spd(r, 5, 10.0), r.standard_normal(5)
    for fam, v in (("one NaN", np.nan), ("one +inf", np.inf)):
        gg = g.copy()
        gg[2] = v
        B.add("non-finite: " + fam, _ldlt_record(5, S, gg))                  # in b: the factor is fine, x carries it
    B.add("non-finite: all inf", _ldlt_record(5, np.full((5, 5), np.inf), np.full(5, np.inf)))
    for n in (0.0, 10.0, 2.5, np.nan):
        B.add("n refused", np.concatenate([[n], np.ones(90)]))


@functools.lru_cache(maxsize=None)
def records(op):
    """(records [n, in_width(op)], the family of each)"""
    B = _Records(op)
    if op == "tv_svd3":
        _square_float(B, 3)
    elif op == "np_null_vector":
        _square_float(B, 4)
    elif op in ("tv_inverse3", "tv_det3"):
        _tv3(B)
    elif op in ("tv_null_vector_8", "tv_null_vector_16"):
        _tv_null(B, 8 if op.endswith("8") else 16)
    elif op == "sim3_largest_eigenvector":
        _sim3_eig(B)
    elif op == "sim3_rotation_of_quaternion":
        _quaternion(B)
    elif op == "mlpnp_rank3":
        _rank3(B)
    elif op == "mlpnp_eig3":
        _eig3(B)
    elif op == "mlpnp_solve6":
        _solve6(B)
    elif op in ("mlpnp_null_vector_12", "mlpnp_null_vector_9"):
        _mlpnp_null(B, 12 if op.endswith("12") else 9)
    elif op == "inertial_ldlt":
        _ldlt(B)
    rec = np.array(B.rec)
    rec.setflags(write=False)
    return rec, tuple(B.fam)


# ----------------------------------------------------------------------------------- files of tests/decomp_probe_main.cc
def write_blocks(path, blocks):
    """blocks: [(op, records [n, in_width(op)])]"""
    with open(path, "wb") as f:
        f.write(struct.pack("=i", len(blocks)))
        for op, rec in blocks:
            rec = np.ascontiguousarray(rec, F64).reshape(-1, IN_WIDTH[op])
            f.write(struct.pack("=ii", OPS.index(op), len(rec)))
            f.write(rec.tobytes())


def read_blocks(path, blocks):
    raw = np.fromfile(path, F64)
    out, at = [], 0
    for op, rec in blocks:
        n = len(np.asarray(rec).reshape(-1, IN_WIDTH[op]))
        out.append(raw[at:at + n * DECOMP_OUT].reshape(n, DECOMP_OUT).copy())
        at += n * DECOMP_OUT
    assert at == len(raw), (at, len(raw))
    return out


def same_bits(a, b):
    """equal bit for bit, a NaN matching any NaN at the same position (its payload and sign are not the routine's)"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def differing_records(a, b):
    return [i for i in range(len(a)) if not same_bits(a[i], b[i])]


# ------------------------------------------------------------------------------------------------ measures, D and the judge
# A measure is a non-negative number that is 0 for an exact answer and does not depend on which of several valid answers (a sign,
# a basis of a repeated value's space) was picked.  Float ops are measured in float64 against float64 LAPACK (1e-16 is far below a
# float's eps); double ops against mpmath at 50 digits, the residuals formed in mpmath too.

def judged_by_measure(op, fam):
    """layer (a) applies: the family is finite, inside the routine's domain, and its answer is decided"""
    if fam.startswith("non-finite") or fam in ("scale: nothing rotates", "near the rule", "integer: coplanar", "singular", "pivot: zero",
                                               "pivot: NaN", "n refused"):
        return False
    return not (op == "inertial_ldlt" and fam == "pivot: negative") and op != "mlpnp_rank3"


SEPARATED = ("separated",)      # a gap of at least 0.1 sigma_1 defines the vector: the angle to the exact one is judged too


def _rel(num, den):
    return 0.0 if num == 0 else (float("inf") if den == 0 else float(num / den))


@functools.lru_cache(maxsize=None)
def _mp():
    """a context of this module's own at 50 digits: the global one's precision belongs to whoever set it"""
    import mpmath
    ctx = mpmath.mp.clone()
    ctx.dps = 50
    return ctx


@functools.lru_cache(maxsize=None)
def _exact_sym(op, i):
    """(eigenvalues ascending, eigenvectors as columns) of record i's symmetric matrix, in mpmath"""
    mp = _mp()
    n = DIM[op]
    M = mp.matrix(records(op)[0][i][:n * n].reshape(n, n).tolist())
    E, Q = mp.eigsy(M)
    order = sorted(range(n), key=lambda k: E[k])
    return [E[k] for k in order], [[Q[r, k] for r in range(n)] for k in order]


def _angle(x, v):
    """the sine of the angle between x and the unit vector v, up to sign"""
    x, v = np.asarray(x, F64), np.asarray(v, F64)
    n = np.linalg.norm(x)
    return float(np.linalg.norm(x - (x @ v) * v) / n) if n > 0 else float("inf")


def _det3_exact(M):
    from fractions import Fraction
    m = [Fraction(float(v)) for v in M]
    terms = [m[0] * m[4] * m[8], -m[0] * m[5] * m[7], -m[1] * m[3] * m[8], m[1] * m[5] * m[6], m[2] * m[3] * m[7], -m[2] * m[4] * m[6]]
    return sum(terms), sum(abs(t) for t in terms)


def _quaternion_exact(q):
    w, x, y, z = (LD(v) for v in q)
    n2 = w * w + x * x + y * y + z * z
    two = LD(2)
    R = [1 - two * (y * y + z * z) / n2, two * (x * y - w * z) / n2, two * (x * z + w * y) / n2,
         two * (x * y + w * z) / n2, 1 - two * (x * x + z * z) / n2, two * (y * z - w * x) / n2,
         two * (x * z - w * y) / n2, two * (y * z + w * x) / n2, 1 - two * (x * x + y * y) / n2]
    S = [1 + two * (y * y + z * z) / n2, two * (abs(x * y) + abs(w * z)) / n2, two * (abs(x * z) + abs(w * y)) / n2,
         two * (abs(x * y) + abs(w * z)) / n2, 1 + two * (x * x + z * z) / n2, two * (abs(y * z) + abs(w * x)) / n2,
         two * (abs(x * z) + abs(w * y)) / n2, two * (abs(y * z) + abs(w * x)) / n2, 1 + two * (x * x + y * y) / n2]
    return np.array(R, LD), np.array(S, LD)


def _solve_measure(S, g, x):
    S, g, x = (np.asarray(v, LD) for v in (S, g, x))
    num, den = np.abs(S @ x - g), np.abs(S) @ np.abs(x) + np.abs(g)
    return max(_rel(a, b) for a, b in zip(num, den))


def ldlt_parts(rec):
    n = int(rec[0])
    U = np.triu(rec[1:1 + n * n].reshape(n, n))
    return n, U + np.triu(U, 1).T, rec[1 + n * n:1 + n * n + n]


def measures(op, i, out):
    """{measure: value} of the output `out` (24 doubles) for record i of op; a non-finite output where a finite one is due gives inf"""
    rec, fam = records(op)[0][i], records(op)[1][i]
    with np.errstate(all="ignore"):
        m = _measures(op, i, rec, fam, np.asarray(out, F64))
    return {k: (v if v == v else float("inf")) for k, v in m.items()}


def _measures(op, i, rec, fam, out):
    if op == "tv_inverse3":
        M, inv = rec.reshape(3, 3), out[:9].reshape(3, 3)
        s = np.linalg.svd(M, compute_uv=False)
        return {"residual / cond": float(np.abs(M @ inv - np.eye(3)).max() / (s[0] / s[2]))}
    if op == "tv_det3":
        exact, sumabs = _det3_exact(rec)
        from fractions import Fraction
        return {"distance": _rel(abs(Fraction(float(out[0])) - exact), sumabs) if np.isfinite(out[0]) else float("inf")}
    if op == "tv_svd3":
        A, U, S, V = rec.reshape(3, 3), out[:9].reshape(3, 3), out[9:12], out[12:21].reshape(3, 3)
        s = np.linalg.svd(A, compute_uv=False)
        return {"reconstruction": _rel(np.abs((U * S) @ V.T - A).max(), s[0]), "U orthogonal": float(np.abs(U.T @ U - np.eye(3)).max()),
                "V orthogonal": float(np.abs(V.T @ V - np.eye(3)).max()), "singular values": _rel(np.abs(S - s).max(), s[0])}
    if op in ("tv_null_vector_8", "tv_null_vector_16", "np_null_vector"):
        n = DIM[op]
        A, x = rec.reshape(-1, n), out[:n]
        _, s, Vt = np.linalg.svd(A, full_matrices=True)
        smin = s[n - 1] if len(s) == n else 0.0
        m = {"unit": abs(float(np.linalg.norm(x)) - 1.0), "residual": _rel(max(0.0, np.linalg.norm(A @ x) - smin), s[0])}
        if fam in SEPARATED:
            m["angle"] = _angle(x, Vt[-1])
        return m
    if op == "sim3_largest_eigenvector":
        A, x = rec.reshape(4, 4), out[:4]
        lam, Q = np.linalg.eigh(A)
        mabs = np.abs(lam).max()
        m = {"unit": abs(float(np.linalg.norm(x)) - 1.0), "Rayleigh": _rel(abs(lam[-1] - x @ A @ x), mabs),
             "residual": _rel(np.linalg.norm(A @ x - lam[-1] * x), mabs)}
        if fam in SEPARATED:
            m["angle"] = _angle(x, Q[:, -1])
        return m
    if op == "sim3_rotation_of_quaternion":
        R, S = _quaternion_exact(rec)
        return {"distance": max(_rel(abs(LD(a) - b), c) for a, b, c in zip(out[:9], R, S))}
    if op == "mlpnp_eig3":
        mp = _mp()
        lam, vec = _exact_sym(op, i)
        mabs = max(abs(v) for v in lam)
        if not np.isfinite(out[:9]).all():
            return {"residual": float("inf")}
        M, E = mp.matrix(rec.reshape(3, 3).tolist()), mp.matrix(out[:9].reshape(3, 3).tolist())
        G = E * E.T
        r = [(E[k, :] * M * E[k, :].T)[0] for k in range(3)]
        res = max(mp.norm(M * E[k, :].T - r[k] * E[k, :].T) for k in range(3))
        m = {"residual": _rel(res, mabs), "orthogonal": float(max(abs(G[a, b] - (a == b)) for a in range(3) for b in range(3))),
             "eigenvalues": _rel(max(abs(r[k] - lam[k]) for k in range(3)), mabs),
             "order": _rel(max(max(mp.mpf(0), r[k] - r[k + 1]) for k in range(2)), mabs)}
        if fam in SEPARATED:
            m["angle"] = max(_angle(out[3 * k:3 * k + 3], [float(v) for v in vec[k]]) for k in range(3))
        return m
    if op in ("mlpnp_null_vector_12", "mlpnp_null_vector_9"):
        mp = _mp()
        n = DIM[op]
        lam, vec = _exact_sym(op, i)
        k = min(range(n), key=lambda j: abs(lam[j]))
        mabs = max(abs(v) for v in lam)
        if not np.isfinite(out[:n]).all():
            return {"residual": float("inf")}
        W, x = mp.matrix(rec.reshape(n, n).tolist()), mp.matrix(out[:n].tolist())
        m = {"unit": float(abs(mp.norm(x) - 1)), "residual": _rel(max(mp.mpf(0), mp.norm(W * x) - abs(lam[k])), mabs)}
        if fam in SEPARATED:
            m["angle"] = _angle(out[:n], [float(v) for v in vec[k]])
        return m
    if op == "mlpnp_solve6":
        return {"backward error": _solve_measure(rec[:36].reshape(6, 6), rec[36:42], out[:6])}
    if op == "inertial_ldlt":
        n, S, b = ldlt_parts(rec)
        return {"backward error": _solve_measure(S, b, out[1:1 + n])}
    return {}


def lapack(op, i):
    """the 24 outputs of record i as numpy's LAPACK gives them in the op's precision (None where it refuses)"""
    rec, o = records(op)[0][i], np.zeros(DECOMP_OUT)
    f = F32 if op in FLOAT_OPS else F64
    try:
        with np.errstate(all="ignore"):
            if op == "tv_inverse3":
                o[:9] = np.linalg.inv(rec.reshape(3, 3).astype(f)).reshape(-1)
            elif op == "tv_det3":
                o[0] = np.linalg.det(rec.reshape(3, 3).astype(f))
            elif op == "tv_svd3":
                U, S, Vt = np.linalg.svd(rec.reshape(3, 3).astype(f))
                o[:9], o[9:12], o[12:21] = U.reshape(-1), S, Vt.T.reshape(-1)
            elif op in ("tv_null_vector_8", "tv_null_vector_16", "np_null_vector"):
                n = DIM[op]
                o[:n] = np.linalg.svd(rec.reshape(-1, n).astype(f), full_matrices=True)[2][-1]
            elif op == "sim3_largest_eigenvector":
                o[:4] = np.linalg.eigh(rec.reshape(4, 4).astype(f))[1][:, -1]
            elif op == "sim3_rotation_of_quaternion":                       # no LAPACK routine: the same rotation by another float formula
                w, x, y, z = rec.astype(f)
                s = f(2) / (w * w + x * x + y * y + z * z)
                o[:9] = [f(1) - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y), s * (x * y + w * z), f(1) - s * (x * x + z * z),
                         s * (y * z - w * x), s * (x * z - w * y), s * (y * z + w * x), f(1) - s * (x * x + y * y)]
            elif op == "mlpnp_eig3":
                o[:9] = np.linalg.eigh(rec.reshape(3, 3))[1].T.reshape(-1)
            elif op in ("mlpnp_null_vector_12", "mlpnp_null_vector_9"):
                n = DIM[op]
                lam, Q = np.linalg.eigh(rec.reshape(n, n))
                o[:n] = Q[:, int(np.argmin(np.abs(lam)))]
            elif op == "mlpnp_solve6":
                o[:6] = np.linalg.solve(rec[:36].reshape(6, 6), rec[36:42])
            elif op == "inertial_ldlt":
                n, S, b = ldlt_parts(rec)
                o[0], o[1:1 + n] = 1.0, np.linalg.solve(S, b)
            else:
                return None
    except np.linalg.LinAlgError:
        return None
    return o


def record_dim(op, i):
    return int(records(op)[0][i][0]) if op == "inertial_ldlt" else DIM[op]


@functools.lru_cache(maxsize=None)
def measure(op):
    """{family: {measure: D}}: the largest value LAPACK in the same precision reaches on the family, floored at n eps"""
    fams = records(op)[1]
    D = {}
    for i, fam in enumerate(fams):
        if not judged_by_measure(op, fam):
            continue
        o = lapack(op, i)
        m = measures(op, i, o) if o is not None else {}
        floor = record_dim(op, i) * eps_of(op)
        d = D.setdefault(fam, {})
        for k in measures(op, i, np.zeros(DECOMP_OUT)):
            v = m.get(k, 0.0)
            d[k] = max(d.get(k, 0.0), floor, v if np.isfinite(v) else 0.0)
    return D


@functools.lru_cache(maxsize=None)
def sweeps(op):
    """{family: the most rotating sweeps the restatement needs on a record of the family}"""
    if op not in SWEEP_CAP:
        return {}
    fams, traces = records(op)[1], restated_all(op)[1]
    S = {}
    for fam, tr in zip(fams, traces):
        S[fam] = max(S.get(fam, 0), tr.get("sweeps", 0))
    return S


def sweep_cap_exempt(op, fam):
    """families outside the routine's domain, where the cap is what ends the iteration"""
    return fam.startswith("non-finite") or fam == "scale: below the domain"


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


EXPECTED_RANK = {"integer: rank 0": 0, "integer: rank 1": 1, "integer: rank 2": 2, "integer: rank 3": 3, "permutation": 3,
                 "clear gap: rank 3": 3, "scale": 3, "on the rule": 1}


def _is_unit_vector(x, at=None):
    x = np.asarray(x)
    return np.count_nonzero(x) == 1 and x.max() == 1.0 and (at is None or x[at] == 1.0)


def exact_failures(op, i, out):
    """what must hold exactly: orders, signs, flags, ranks, the documented outcome of a non-finite or out-of-domain record"""
    rec, fam = records(op)[0][i], records(op)[1][i]
    bad = []
    finite = not fam.startswith("non-finite")
    if not np.all(out[{**COOPERATIVE, "tv_svd3": 21, "inertial_ldlt": 10}.get(op, DIM[op] if op not in ("tv_det3", "mlpnp_rank3") else 1) + 1:] == 0):
        if op not in ("tv_inverse3", "sim3_rotation_of_quaternion", "mlpnp_eig3", "mlpnp_solve6"):
            bad.append("an output slot the op does not write is not 0")
    if op in COOPERATIVE and out[COOPERATIVE[op]] != 0:
        bad.append(f"{out[COOPERATIVE[op]]:.0f} lanes differ from lane 0")
    if op == "tv_svd3" and finite:
        S = out[9:12]
        if not (S[0] >= S[1] >= S[2] >= 0):
            bad.append(f"S is not descending and non-negative: {S}")
    if op == "mlpnp_rank3" and fam in EXPECTED_RANK and out[0] != EXPECTED_RANK[fam]:
        bad.append(f"rank {out[0]:.0f}, exactly {EXPECTED_RANK[fam]}")
    if op == "inertial_ldlt":
        n = int(rec[0]) if fam != "n refused" else 0
        want = -1.0 if fam == "n refused" else 0.0 if fam.startswith("pivot") or fam == "non-finite: all inf" else 1.0
        if out[0] != want:
            bad.append(f"ok {out[0]}, expected {want}")
        if want != 1.0 and np.any(out[1:] != 0):
            bad.append("x was touched on a refusal")
        if want == 1.0 and finite and not np.isfinite(out[1:1 + n]).all():
            bad.append("x is not finite")
    if op in ("tv_null_vector_8", "tv_null_vector_16"):
        if fam == "scale: nothing rotates" and not _is_unit_vector(out[:9]):
            bad.append("outside the domain nothing rotates: x is a unit vector of the basis")
        if fam == "non-finite: all inf" and not _is_unit_vector(out[:9], 0):
            bad.append("an all-infinite A rotates nothing and returns the first unit vector")
    if op == "sim3_largest_eigenvector" and fam == "non-finite: all inf" and not _is_unit_vector(out[:4], 0):
        bad.append("an all-infinite A rotates nothing and returns the first unit vector")
    return bad


def judge(op, out, D=None):
    """(largest measure / D over the judged records, failures) of the outputs [n, 24] of every record of op"""
    D = golden()["D"].get(op, {}) if D is None else D
    fams = records(op)[1]
    worst, failures = 0.0, []
    for i, fam in enumerate(fams):
        failures += [(i, fam, what) for what in exact_failures(op, i, out[i])]
        if not judged_by_measure(op, fam):
            continue
        for k, v in measures(op, i, out[i]).items():
            ratio = v / D[fam][k]
            worst = max(worst, ratio)
            if not ratio <= FACTOR:
                failures.append((i, fam, f"{k} {v:.3g} = {ratio:.3g} D"))
    return worst, failures


def measure_all():
    return {"D": {op: measure(op) for op in OPS if measure(op)}, "sweeps": {op: sweeps(op) for op in OPS if sweeps(op)}}


if __name__ == "__main__":
    if sys.argv[1:] == ["--write-golden"]:
        with open(GOLDEN, "w") as f:
            json.dump(measure_all(), f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", GOLDEN)
    for op in OPS:
        print(op, len(records(op)[0]), "records; sweeps", sweeps(op))
        for fam, d in measure(op).items():
            print("   ", fam, {k: f"{v:.3g}" for k, v in d.items()})
