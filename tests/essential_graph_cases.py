"""Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1410-1675 and :1677-1985) after its gathering loops, restated in float64
numpy with the g2o pieces it runs (Thirdparty/g2o/g2o: types/sim3.h:70-272, types/se3_ops.hpp:27-47,
types/types_seven_dof_expmap.h:60-69,106-114, core/base_binary_edge.hpp:55-90,131-203,
core/optimization_algorithm_levenberg.cpp:61-195, core/sparse_optimizer.cpp:234,376-389), the scene generator and the scene list of
the GPU tests.  No GPU, no library, and no code shared with ms-slam_amd/csrc/essential_graph_device.h: the edges are evaluated as
arrays, all 29 error vectors of all edges in one pass.

EdgeSim3 has no linearizeOplus, so g2o differentiates it numerically: central differences with delta = 1e-9 through oplus.  A
one-ulp difference in an error entry is 1e-7 in a Jacobian entry, and that noise is drawn again at every estimate, so two
evaluations that differ only in rounding end at estimates that differ by far more than 1e-15.
`python tests/essential_graph_cases.py --measure` measures by how much, over the variants below, and writes
tests/golden/essential_graph_sensitivity.json.

What the restatement fixes where the reference leaves it to Eigen / libm:
  * a product of small matrices is the plain row-by-column sum, left to right, without fused multiply-adds;
  * W.lu().solve(t) is the 3x3 LU with partial pivoting (the first largest entry), the multipliers by division;
  * the 7N system is solved DENSELY in the natural vertex order (the reference: a sparse Cholesky): `solver` = 'ldlt', the
    square-root-free unpivoted L D L^T that fails on a pivot !(d > 0), or 'lapack', numpy's pivoted LU;
  * `sum_order` fixes how H's blocks, b and the cost are added over the active edges: 'forward' (g2o's edge list), 'reverse',
    'pairwise' (a balanced tree);
  * `nudge` moves the results of log, acos, sin, cos and exp up by one ulp: what another libm may return.
"""
import hashlib
import json
import math
import os
import sys

import numpy as np

from sim3_opt_cases import sim3_exp   # Sim3(update), scalar: one call per vertex and trial

F64 = np.float64
DBL_MAX = sys.float_info.max
DELTA = 1e-9                       # base_binary_edge.hpp:147
SCALAR = 1.0 / (2 * DELTA)         # :148
LAMBDA_INIT = 1e-16                # setUserLambdaInit (Optimizer.cc:1423, :1698)
ITERATIONS = 20                    # optimize(20) (:1629, :1933)
VARIANTS = (("forward", False, "ldlt"), ("reverse", False, "ldlt"), ("pairwise", False, "ldlt"), ("forward", True, "ldlt"),
            ("forward", False, "lapack"))   # (sum_order, nudge, solver); the first is THE restatement
MARGIN = 16                        # the project's margin over the measured spread (DESIGN.md sections 10, 14, 16, 17)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "essential_graph_sensitivity.json")


def _up(v, nudge):
    return np.nextafter(v, np.inf) if nudge else v


# ------------------------------------------------------------------------------------------- g2o::Sim3 over arrays [M, 8]: q t s
def _qmul(a, b):
    ax, ay, az, aw = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    bx, by, bz, bw = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    w = ((aw * bw - ax * bx) - ay * by) - az * bz
    x = ((aw * bx + ax * bw) + ay * bz) - az * by
    y = ((aw * by + ay * bw) + az * bx) - ax * bz
    z = ((aw * bz + az * bw) + ax * by) - ay * bx
    return np.stack([x, y, z, w], 1)


def _qrot(q, v):
    """Eigen's Quaternion * Vector3: uv = 2 vec x v; v + w uv + vec x uv"""
    qx, qy, qz, qw = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    X, Y, Z = v[:, 0], v[:, 1], v[:, 2]
    ux, uy, uz = qy * Z - qz * Y, qz * X - qx * Z, qx * Y - qy * X
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return np.stack([(X + qw * ux) + (qy * uz - qz * uy), (Y + qw * uy) + (qz * ux - qx * uz), (Z + qw * uz) + (qx * uy - qy * ux)], 1)


def sim_mul(a, b):
    """Sim3::operator* (sim3.h:266-272)"""
    s = a[:, 7:8]
    return np.concatenate([_qmul(a, b), s * _qrot(a, b[:, 4:7]) + a[:, 4:7], s * b[:, 7:8]], 1)


def sim_inv(a):
    """Sim3::inverse (sim3.h:233-236)"""
    qc = a[:, :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    f = -1.0 / a[:, 7:8]
    return np.concatenate([qc, _qrot(qc, f * a[:, 4:7]), 1.0 / a[:, 7:8]], 1)


def _lu3_solve(W, t):
    """PartialPivLU of [M, 3, 3] and the two substitutions"""
    W, y = W.copy(), t.copy()
    idx = np.arange(len(W))
    for k in range(3):
        p = np.argmax(np.abs(W[:, k:, k]), axis=1) + k     # (the first largest)
        rk, rp = W[idx, k].copy(), W[idx, p].copy()
        W[idx, k], W[idx, p] = rp, rk
        yk, yp = y[idx, k].copy(), y[idx, p].copy()
        y[idx, k], y[idx, p] = yp, yk
        for i in range(k + 1, 3):
            W[:, i, k] = W[:, i, k] / W[:, k, k]
            for j in range(k + 1, 3):
                W[:, i, j] = W[:, i, j] - W[:, i, k] * W[:, k, j]
    y[:, 1] = y[:, 1] - W[:, 1, 0] * y[:, 0]
    y[:, 2] = y[:, 2] - W[:, 2, 0] * y[:, 0]
    y[:, 2] = y[:, 2] - W[:, 2, 1] * y[:, 1]
    x = np.empty_like(y)
    x[:, 2] = y[:, 2] / W[:, 2, 2]
    y[:, 0] = y[:, 0] - W[:, 0, 2] * x[:, 2]
    y[:, 1] = y[:, 1] - W[:, 1, 2] * x[:, 2]
    x[:, 1] = y[:, 1] / W[:, 1, 1]
    y[:, 0] = y[:, 0] - W[:, 0, 1] * x[:, 1]
    x[:, 0] = y[:, 0] / W[:, 0, 0]
    return x


def log_branches(S):
    """which of Sim3::log's four branches each row takes: 2 * (sigma != 0 branch) + (theta branch)"""
    qx, qy, qz = S[:, 0], S[:, 1], S[:, 2]
    d = 0.5 * ((((1 - (2 * qy * qy + 2 * qz * qz)) + (1 - (2 * qx * qx + 2 * qz * qz))) + (1 - (2 * qx * qx + 2 * qy * qy))) - 1)
    return 2 * (np.abs(np.log(S[:, 7])) >= 0.00001) + (~(d > 1 - 0.00001))


def sim_log(S, nudge=False):
    """Sim3::log (sim3.h:148-230) -> [M, 7]"""
    qx, qy, qz, qw, s = S[:, 0], S[:, 1], S[:, 2], S[:, 3], S[:, 7]
    with np.errstate(all="ignore"):
        sigma = np.where(s == 1.0, 0.0, _up(np.log(s), nudge))                 # :151 (log(1) is 0 in every libm)
        tx, ty, tz = 2 * qx, 2 * qy, 2 * qz                                    # :160 toRotationMatrix
        twx, twy, twz, txx, txy, txz = tx * qw, ty * qw, tz * qw, tx * qx, ty * qx, tz * qx
        tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
        R00, R01, R02 = 1 - (tyy + tzz), txy - twz, txz + twy
        R10, R11, R12 = txy + twz, 1 - (txx + tzz), tyz - twx
        R20, R21, R22 = txz - twy, tyz + twx, 1 - (txx + tyy)
        d = 0.5 * (((R00 + R11) + R22) - 1)                                    # :161
        dR = np.stack([R21 - R12, R02 - R20, R10 - R01], 1)                    # deltaR
        eps = 0.00001
        small = d > 1 - eps
        theta = _up(np.arccos(np.where(small, 0.0, d)), nudge)
        f = np.where(small, 0.5, theta / (2 * np.sqrt(1 - d * d)))             # :174, :183
        om = f[:, None] * dR
        theta2 = theta * theta
        sn, cs = _up(np.sin(theta), nudge), _up(np.cos(theta), nudge)
        sig0 = np.abs(sigma) < eps                                             # :169
        sigma2 = sigma * sigma
        C = np.where(sig0, 1.0, (s - 1) / sigma)                               # :171, :191
        a, b, c = s * sn, s * cs, theta2 + sigma * sigma                       # :207-209
        A = np.where(sig0, np.where(small, 0.5, (1 - cs) / theta2),
                     np.where(small, ((sigma - 1) * s + 1) / sigma2, (a * sigma + (1 - b) * theta) / (theta * c)))
        B = np.where(sig0, np.where(small, 1. / 6., (theta - sn) / (theta2 * theta)),
                     np.where(small, (((0.5 * sigma2 - sigma) + 1) * s) / (sigma2 * sigma),
                              ((C - ((b - 1) * sigma + a * theta) / c) * 1.) / theta2))
    z = np.zeros_like(s)
    O = np.stack([np.stack([z, -om[:, 2], om[:, 1]], 1), np.stack([om[:, 2], z, -om[:, 0]], 1), np.stack([-om[:, 1], om[:, 0], z], 1)], 1)
    W = np.empty_like(O)
    for i in range(3):                                                         # :215: A*Omega + (B*Omega)*Omega + C*I
        for j in range(3):
            p = ((B * O[:, i, 0]) * O[:, 0, j] + (B * O[:, i, 1]) * O[:, 1, j]) + (B * O[:, i, 2]) * O[:, 2, j]
            W[:, i, j] = (A * O[:, i, j] + p) + C * (1.0 if i == j else 0.0)
    ups = _lu3_solve(W, S[:, 4:7])                                             # :217
    return np.concatenate([om, ups, sigma[:, None]], 1)


def edge_errors(C, v0, v1, nudge=False):
    """EdgeSim3::computeError over arrays: (C * v0 * v1^-1).log()"""
    return sim_log(sim_mul(sim_mul(C, v0), sim_inv(v1)), nudge)


def _sim_of(q, t, s):
    return np.array([[*q, *t, s]], F64)


def perturbation_table(nudge):
    """Sim3(+-delta e_d) for d = 0..6 (entry 2 d, 2 d + 1) and Sim3(0) (entry 14)"""
    tab = []
    for k in range(15):
        u = [0.0] * 7
        if k < 14:
            u[k >> 1] = -DELTA if k & 1 else DELTA
        tab.append(_sim_of(*sim3_exp(u, nudge))[0])
    return np.array(tab)


# ------------------------------------------------------------------------------------------------------------------ the sums
def ordered_sum(terms, order):
    terms = list(terms)
    if order == "reverse":
        terms = terms[::-1]
    if order == "pairwise":
        while len(terms) > 1:
            terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
        return terms[0]
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


def ldlt_solve(S, b, block=64):
    """S x = b by L D L^T without pivoting and without a square root; (x, ok): ok False on a pivot !(d > 0).  Right-looking in panels:
    the entries see the same subtractions as column by column, in panel-sized groups"""
    S = S.copy()
    n = len(b)
    d = np.zeros(n)
    for j0 in range(0, n, block):
        j1 = min(n, j0 + block)
        for j in range(j0, j1):
            d[j] = S[j, j]
            if not d[j] > 0:
                return None, False
            v = S[j + 1:, j].copy()
            l = v * (1.0 / d[j])
            S[j + 1:, j] = l
            if j + 1 < j1:
                S[j + 1:, j + 1:j1] -= np.outer(l, v[:j1 - j - 1])
        if j1 < n:
            L21 = S[j1:, j0:j1]
            S[j1:, j1:] -= (L21 * d[j0:j1]) @ L21.T
    L = np.tril(S, -1)
    y = b.copy()
    for j in range(n):
        y[j + 1:] -= L[j + 1:, j] * y[j]
    x = y / d
    for j in range(n - 1, -1, -1):
        x[:j] -= L[j, :j] * x[j]
    return x, True


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


def linearise(sc, est, act, free_of, tab, order, nudge):
    """computeActiveErrors, activeRobustChi2, buildSystem -> (cost, H dense [n, n], b [n])"""
    v0, v1 = sc["v0"][act], sc["v1"][act]
    C, E = sc["meas"][act], len(act)
    fs = sc["fix_scale"]
    # the 29 states of every edge in one pass
    a0, a1 = np.repeat(est[v0][None], 29, 0), np.repeat(est[v1][None], 29, 0)
    for k in range(14):
        t0 = np.where((fs[v0] != 0)[:, None] & (k >> 1 == 6), tab[14][None], tab[k][None])
        t1 = np.where((fs[v1] != 0)[:, None] & (k >> 1 == 6), tab[14][None], tab[k][None])
        a0[1 + k] = sim_mul(t0, est[v0])                                       # oplus: Sim3(update) * estimate
        a1[15 + k] = sim_mul(t1, est[v1])
    err = edge_errors(np.tile(C, (29, 1)), a0.reshape(-1, 8), a1.reshape(-1, 8), nudge).reshape(29, E, 7)
    e = err[0]
    chi = e[:, 0] * e[:, 0]
    for d in range(1, 7):
        chi = chi + e[:, d] * e[:, d]
    cost = ordered_sum(chi, order) if E else 0.0
    J = [np.stack([SCALAR * (err[1 + 14 * side + 2 * c] - err[2 + 14 * side + 2 * c]) for c in range(7)], 2) for side in (0, 1)]   # [E, d, col]

    def prod(X, Y):   # X^T Y per edge, the sum over d left to right
        acc = X[:, 0, :, None] * Y[:, 0, None, :]
        for d in range(1, 7):
            acc = acc + X[:, d, :, None] * Y[:, d, None, :]
        return acc

    def rhs(X):       # X^T (-e)
        acc = X[:, 0, :] * -e[:, 0, None]
        for d in range(1, 7):
            acc = acc + X[:, d, :] * -e[:, d, None]
        return acc

    Hxx, bx, Hab = [prod(J[0], J[0]), prod(J[1], J[1])], [rhs(J[0]), rhs(J[1])], prod(J[0], J[1])
    Kf = int((free_of >= 0).sum())
    n = 7 * Kf
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
        H[7 * i:7 * i + 7, 7 * i:7 * i + 7] = ordered_sum(terms, order)
        b[7 * i:7 * i + 7] = ordered_sum(rh[i], order)
    for (i, j), terms in off.items():
        blk = ordered_sum(terms, order)
        H[7 * i:7 * i + 7, 7 * j:7 * j + 7] = blk
        H[7 * j:7 * j + 7, 7 * i:7 * i + 7] = blk.T
    return cost, H, b


def cost_at(sc, est, act, order, nudge):
    if not len(act):
        return 0.0
    e = edge_errors(sc["meas"][act], est[sc["v0"][act]], est[sc["v1"][act]], nudge)
    chi = e[:, 0] * e[:, 0]
    for d in range(1, 7):
        chi = chi + e[:, d] * e[:, d]
    return ordered_sum(chi, order)


def optimize(sc, variant=VARIANTS[0], iterations=ITERATIONS, trace=None):
    """optimizer.optimize(20): sparse_optimizer.cpp:376-389 over levenberg.cpp:61-170 -> dict(estimates [N, 8], status, iterations,
    trials, rejected_trials, solver_failures, stop, chi2_initial, chi2_final, lambda_final)"""
    order, nudge, solver = variant
    est = sc["est"].copy()
    act, free_of, vof = active_set(sc)
    tab = perturbation_table(nudge)
    r = dict(status=0, iterations=0, trials=0, rejected_trials=0, solver_failures=0, stop=0, chi2_initial=0.0, chi2_final=0.0, lambda_final=0.0)
    lam, ni, n_bad, ok = 0.0, 2.0, 0, len(act) > 0
    it = 0
    while it < iterations and ok:
        current, H, b = linearise(sc, est, act, free_of, tab, order, nudge)
        if trace is not None:
            trace.append(dict(H=H, b=b, cost=current))
        ini = current
        if it == 0:
            r["chi2_initial"] = current
            lam, ni, n_bad = LAMBDA_INIT, 2.0, 0
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
            trial = est.copy()
            for i, k in enumerate(vof):                                        # update (sparse_optimizer.cpp:422-441)
                if sc["fix_scale"][k]:
                    x[7 * i + 6] = 0.0                                         # oplusImpl writes into the solver's x
                trial[k] = sim_mul(_sim_of(*sim3_exp([float(v) for v in x[7 * i:7 * i + 7]], nudge)), est[k:k + 1])[0]
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
                est = trial
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
    r["estimates"] = est
    return r


COUNTS = ("status", "iterations", "trials", "rejected_trials", "solver_failures", "stop")


def counts(r):
    return tuple(int(r[k]) for k in COUNTS)


def estimate_difference(a, b):
    """the largest difference of an entry of two estimate arrays; a translation's is taken relative to the largest translation"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    if not len(a):
        return 0.0
    tscale = max(1.0, float(np.abs(b[:, 4:7]).max()))
    return float(max(np.abs(a[:, :4] - b[:, :4]).max(), np.abs(a[:, 4:7] - b[:, 4:7]).max() / tscale, np.abs(a[:, 7] - b[:, 7]).max()))


# --------------------------------------------------------------------------------------------------------------- the scenes
def _rand_sim(rng, rot, trans, sig):
    u = np.concatenate([rng.normal(0, 1, 3) * rot, rng.normal(0, 1, 3) * trans, [rng.normal(0, 1) * sig]])
    return _sim_of(*sim3_exp([float(v) for v in u]))


def make_graph(seed, n, edges, fixed, fix_scale, noise=(2e-3, 1e-2, 0.0), perturb=(2e-2, 1e-1, 0.0), drift=0.0, spacing=1.0):
    """n planted poses along a gently turning path; measurements Sji = Sjw Swi from them, times exp(noise); the estimates are
    the planted poses times exp(perturbation) (a fixed vertex keeps the planted pose).  drift: sigma added per vertex to the
    ESTIMATES' scale (a monocular drift), only meaningful with free scale."""
    rng = np.random.default_rng(seed)
    true = np.zeros((n, 8))
    for k in range(n):
        ang = 0.05 * k
        q, t, s = sim3_exp([0.01 * math.sin(k), ang, 0.02 * math.cos(0.7 * k), spacing * k, 0.3 * math.sin(0.3 * k), 0.1 * k, 0.0])
        true[k] = [*q, *t, 1.0]
    fixed = np.array([1 if k in fixed else 0 for k in range(n)], np.int32) if not isinstance(fixed, np.ndarray) else fixed
    fs = np.full(n, fix_scale, np.int32) if np.isscalar(fix_scale) else np.array(fix_scale, np.int32)
    est = true.copy()
    for k in range(n):
        if not fixed[k]:
            p = _rand_sim(rng, perturb[0], perturb[1], 0.0 if fs[k] else perturb[2] + drift * k)
            est[k] = sim_mul(p, true[k:k + 1])[0]
    v0 = np.array([e[0] for e in edges], np.int32)
    v1 = np.array([e[1] for e in edges], np.int32)
    meas = np.zeros((len(edges), 8))
    for e, (i, j) in enumerate(edges):
        m = sim_mul(true[j:j + 1], sim_inv(true[i:i + 1]))                     # Sji = Sjw * Swi (Optimizer.cc:1490-1493)
        if any(noise):
            m = sim_mul(_rand_sim(rng, *noise), m)
        meas[e] = m[0]
    return dict(est=est, fixed=fixed, fix_scale=fs, v0=v0, v1=v1, meas=meas, true=true)


def _chain(n, extra=()):
    return [(k, k + 1) for k in range(n - 1)] + list(extra)


def _scene_log_branches():
    """rotations near identity and near pi / 2 in the base errors, with sigma = 0 exactly (vertices 1, 2: fixed scale, s = 1.0) and
    sigma != 0 (vertices 3, 4: free scale): two measurements that differ by a rotation of pi pull a vertex to pi / 2 from each"""
    sc = make_graph(31, 5, [(0, 1), (0, 2), (0, 2), (0, 3), (0, 4), (0, 4)], {0}, [1, 1, 1, 0, 0], noise=(1e-4, 1e-3, 0.0),
                    perturb=(1e-3, 1e-2, 2e-2))
    half_turn = _sim_of(*sim3_exp([0.0, 0.0, math.pi, 0.0, 0.0, 0.0, 0.0]))
    bigger = _sim_of(*sim3_exp([0.0, 0.0, math.pi, 0.0, 0.0, 0.0, 0.05]))
    sc["meas"][2] = sim_mul(half_turn, sc["meas"][2:3])[0]
    sc["meas"][5] = sim_mul(bigger, sc["meas"][5:6])[0]
    for k in (2, 4):   # start a quarter turn away from both measurements
        q = _sim_of(*sim3_exp([0.0, 0.0, math.pi / 2 + 0.01 * k, 0.0, 0.0, 0.0, 0.0]))
        sc["est"][k] = sim_mul(q, sc["est"][k:k + 1])[0]
    sc["est"][1, 7] = sc["est"][2, 7] = 1.0
    return sc


def _scene_at_optimum():
    sc = make_graph(37, 8, _chain(8, [(0, 7), (2, 6)]), {0}, 1)
    sc["est"] = optimize(sc, iterations=40)["estimates"]
    return sc


def _scene_merge():
    """the merge form's three classes: fixed (_fix_scale set), fixed-corrected and non-fixed (free, the constructor's false)"""
    n = 18
    fixed = {0, 1, 2}
    fs = [1 if k in fixed else 0 for k in range(n)]
    edges = _chain(n, [(0, 9), (1, 12), (4, 15), (2, 17), (0, 1), (1, 2)])
    return make_graph(41, n, edges, fixed, fs, noise=(2e-3, 1e-2, 2e-3), perturb=(2e-2, 1e-1, 2e-2))


def _loops(n, step, seed):
    rng = np.random.default_rng(seed)
    extra = [(k, k - int(rng.integers(2, 6))) for k in range(6, n, step)] + [(0, n - 1)]
    return _chain(n, extra)


_BUILDERS = {
    "one_free": lambda: make_graph(1, 2, [(0, 1)], {0}, 1),
    "six_free": lambda: make_graph(2, 7, _chain(7, [(0, 6), (2, 5)]), {0}, 0, noise=(2e-3, 1e-2, 2e-3), perturb=(2e-2, 1e-1, 2e-2)),
    "seven_free": lambda: make_graph(3, 8, _chain(8, [(0, 7), (1, 5)]), {0}, 1),
    "fourteen_free": lambda: make_graph(4, 15, _chain(15, [(0, 14), (3, 11), (5, 9)]), {0}, 1),
    "chain40_loop": lambda: make_graph(5, 40, _chain(40, [(39, 0)]), {0}, 1),
    "chain40_drift": lambda: make_graph(6, 40, _chain(40, [(39, 0)]), {0}, 0, noise=(2e-3, 1e-2, 2e-3), perturb=(2e-2, 1e-1, 0.0), drift=2e-3),
    "duplicate_edges": lambda: make_graph(7, 6, _chain(6, [(1, 3), (1, 3), (3, 1), (0, 5), (1, 3)]), {0}, 1),
    "hub70": lambda: make_graph(8, 72, [(1, k) if k % 2 else (k, 1) for k in range(2, 72)] + [(0, 1)] + [(k, k + 1) for k in range(2, 71, 5)],
                                {0}, 1, spacing=0.2),
    "active_set": lambda: make_graph(9, 9, _chain(6, [(6, 7), (0, 5)]), {0, 6, 7}, 1),          # (6, 7): both fixed; 8: no edge
    "one_sided": lambda: make_graph(10, 6, [(0, 1), (2, 0), (1, 2), (5, 3), (4, 5), (3, 4), (2, 3)], {0, 5}, 0,
                                    noise=(2e-3, 1e-2, 2e-3), perturb=(2e-2, 1e-1, 2e-2)),
    "log_branches": _scene_log_branches,
    "at_optimum": _scene_at_optimum,
    "merge_classes": _scene_merge,
    "free150_loops": lambda: make_graph(11, 151, _loops(151, 7, 11), {0}, 1, spacing=0.5),
    # fixed scale through the reference's optimize(20) to its own exit: with measurement noise ten times the other scenes' the gain of
    # a step falls below a thousandth of the cost while it is still far above rounding, so _nBad >= 3 ends every variant alike
    "fixed_noisy_20": lambda: make_graph(51, 8, _chain(8, [(0, 7), (1, 5)]), {0}, 1, noise=(2e-2, 1e-1, 0.0)),
    "chain40_noisy_20": lambda: make_graph(54, 40, _chain(40, [(39, 0), (30, 8)]), {0}, 1, noise=(2e-2, 1e-1, 0.0)),
}
GPU_SCENES = tuple(_BUILDERS)
# Once a fixed-scale graph has converged (three or four steps), every further trial moves the cost in its last digits only, and
# whether such a trial is accepted is decided by rounding: the variants then leave the loop by different exits.  These scenes
# therefore run optimize(3), every step of which is a large gain; the others, two noisy fixed-scale graphs among them (the _nBad
# exit after five or six iterations), run the reference's optimize(20) to their exit (ten
# rejected trials for the free-scale graphs, whose second linearisation lands in Sim3::log's small-angle branch with sigma != 0,
# where the reference's B = ((sigma^2 / 2 - sigma + 1) s) / sigma^3 is of order 1e9 and the step is useless: restated, not fixed).
SHORT = ("one_free", "seven_free", "fourteen_free", "chain40_loop", "duplicate_edges", "hub70", "active_set", "free150_loops")
_scene_cache, _ref_cache = {}, {}


def scene(name):
    if name not in _scene_cache:
        _scene_cache[name] = _BUILDERS[name]()
        _scene_cache[name]["iterations"] = 3 if name in SHORT else ITERATIONS
    return _scene_cache[name]


def reference(name, variant=VARIANTS[0]):
    """the restatement's result for a scene, computed once"""
    key = (name, variant)
    if key not in _ref_cache:
        _ref_cache[key] = optimize(scene(name), variant, scene(name)["iterations"])
    return _ref_cache[key]


def consistent_graph(free_scale):
    """measurements taken from the planted poses, estimates perturbed: the optimum has zero cost"""
    return make_graph(21, 10, _chain(10, [(0, 9), (2, 7)]), {0}, 0 if free_scale else 1, noise=(0.0, 0.0, 0.0), perturb=(2e-2, 1e-1, 2e-2))


def digest(sc):
    h = hashlib.sha256()
    for k in ("est", "fixed", "fix_scale", "v0", "v1", "meas"):
        h.update(np.ascontiguousarray(sc[k]).tobytes())
    return h.hexdigest()[:16]


def vertex_records(sc):
    """the scene as msorb.EG_VERTEX_DTYPE-shaped plain arrays: (q, t, s, fixed, fix_scale)"""
    return sc["est"][:, :4], sc["est"][:, 4:7], sc["est"][:, 7], sc["fixed"], sc["fix_scale"]


# ---------------------------------------------------------------------- files of tests/essential_graph_main.cc (native endianness)
def write_scenes(path, scenes):
    """n_scenes | per scene: N E iterations (int32) | est [N, 8] f64 | fixed [N] fix_scale [N] v0 [E] v1 [E] int32 | meas [E, 8] f64"""
    with open(path, "wb") as f:
        f.write(np.array([len(scenes)], np.int32).tobytes())
        for sc in scenes:
            f.write(np.array([len(sc["fixed"]), len(sc["v0"]), sc.get("iterations", ITERATIONS)], np.int32).tobytes())
            f.write(np.ascontiguousarray(sc["est"], F64).tobytes())
            for k in ("fixed", "fix_scale", "v0", "v1"):
                f.write(np.ascontiguousarray(sc[k], np.int32).tobytes())
            f.write(np.ascontiguousarray(sc["meas"], F64).tobytes())


def read_results(path, scenes):
    """per scene: 6 int32 (COUNTS) | chi2_initial chi2_final lambda_final f64 | estimates [N, 8] f64"""
    out = []
    with open(path, "rb") as f:
        for sc in scenes:
            c = np.frombuffer(f.read(24), np.int32)
            d = np.frombuffer(f.read(24), F64)
            n = len(sc["fixed"])
            est = np.frombuffer(f.read(64 * n), F64).reshape(n, 8)
            r = dict(zip(COUNTS, (int(v) for v in c)))
            r.update(chi2_initial=float(d[0]), chi2_final=float(d[1]), lambda_final=float(d[2]), estimates=est)
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
    estimate through.  The floor is one rounding of an entry of size one: a scene on which every variant returns the same bits (the
    start at the optimum, where every trial is rejected) still allows the last bit"""
    return MARGIN * max(golden()["scenes"][name]["spread"], float(np.finfo(F64).eps))


def measure():
    g = dict(scenes={}, D=0.0)
    for name in GPU_SCENES:
        rs = [reference(name, v) for v in VARIANTS]
        cs = {counts(r) for r in rs}
        dd = max(estimate_difference(a["estimates"], b["estimates"]) for a in rs for b in rs)
        g["scenes"][name] = dict(digest=digest(scene(name)), iterations=scene(name)["iterations"], counts=list(counts(rs[0])), variants_agree=len(cs) == 1, spread=dd,
                                 chi2_initial=rs[0]["chi2_initial"], chi2_final=rs[0]["chi2_final"])
        g["D"] = max(g["D"], dd)
        print(name, counts(rs[0]), "agree" if len(cs) == 1 else f"DISAGREE {sorted(cs)}", f"spread {dd:.3e}",
              f"chi2 {rs[0]['chi2_initial']:.3e} -> {rs[0]['chi2_final']:.3e}", flush=True)
    return g


if __name__ == "__main__":
    g = measure()
    if "--measure" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(g, f, indent=1)
            f.write("\n")
    print("D =", g["D"])
