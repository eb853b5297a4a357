"""Optimizer::FullInertialBA (src/Optimizer.cc:366-756) after its gathering loops, restated in float64 / float32 numpy for pinhole
KeyFrames without a second camera: g2o's optimize(its) with setUserLambdaInit(1e-5) over either of its two graphs.  init = 0: pose,
velocity and both biases per KeyFrame, EdgeInertial (Huber sqrt(16.92), the information as given), EdgeGyroRW / EdgeAccRW.  init = 1:
pose and velocity per KeyFrame, ONE gyro and one acc bias (the last non-marginalised unknowns) shared by every EdgeInertial, no
random-walk edge, EdgePriorAcc / EdgePriorGyro with bprior = 0.  The active-edge rule (sparse_optimizer.cpp:227-234), the points
without an edge at a free KeyFrame left out (:677-680), the stop flag where g2o calls terminate(), no classification, no FAIL rule.

The edges' restatements, the records and the scene generator are those of tests/local_inertial_ba_cases.py and
tests/pose_inertial_cases.py; the graph, the system over the unknowns of both forms, the Schur complement, the loop and the scene
list are stated here.  No GPU, no library and no code shared with ms-slam_amd/csrc/full_inertial_ba_device.h.

`python tests/full_inertial_ba_cases.py --measure` writes tests/golden/full_inertial_ba_sensitivity.json: D per quantity is the
largest difference between the first of VARIANTS (THE restatement) and any other over the scene list, reported also for the scenes
without a fixed KeyFrame alone (`D_no_fixed`) and for the others (`D_fixed`)."""
import functools
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from inertial_opt_cases import DBL_MAX, F32, F64, _rot, ordered_sum  # noqa: E402
import local_inertial_ba_cases as lc  # noqa: E402
import pose_inertial_cases as pic  # noqa: E402

MARGIN = lc.MARGIN
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "full_inertial_ba_sensitivity.json")
VARIANTS = lc.VARIANTS
QUANTITIES = ("Rwb", "twb", "v", "bg", "ba", "points", "cost")
CAPACITY = {0: 477, 1: 795}
PRIORS = ((1e2, 1e10), (1e2, 1e5), (1.0, 1e5))                                 # InitializeIMU's (priorG, priorA), LocalMapping.cc:185-213

FIBA_PROBLEM_DTYPE = np.dtype([("init", "<i4"), ("iterations", "<i4"), ("prior_g", "<f4"), ("prior_a", "<f4"), ("bg0", "<f8", 3), ("ba0", "<f8", 3)])
assert FIBA_PROBLEM_DTYPE.itemsize == 64


# ------------------------------------------------------------------------------------------------ the graph
def graph(sc):
    """the vertices and the active edges of one call"""
    init = int(sc["init"])
    kind = sc["kf"]["kind"]
    free = np.flatnonzero(kind == 0)
    free_of = np.full(len(kind), -1)
    free_of[free] = np.arange(len(free))
    Kf, per = len(free), (3 if init else 9)
    idx = [np.concatenate([6 * i + np.arange(6), 6 * Kf + per * i + np.arange(per)]) for i in range(Kf)]
    nb = (6 + per) * Kf
    n = nb + (6 if init else 0)
    P = len(sc["pos"])
    included = np.zeros(P, bool)
    if len(sc["edge_kf"]):
        included[sc["edge_pt"][free_of[sc["edge_kf"]] >= 0]] = True           # :596-598, :677-680
    keep = included[sc["edge_pt"]] if len(sc["edge_pt"]) else np.zeros(0, bool)
    new_of = np.cumsum(included) - 1
    sub = dict(sc, pos=sc["pos"][included], edge_kf=sc["edge_kf"][keep], edge_pt=new_of[sc["edge_pt"][keep]].astype(np.int64),
               xy=sc["xy"][keep], ur=sc["ur"][keep], inv=sc["inv"][keep])
    active = [bool(init) or free_of[int(E["pre"]["kf_prev"])] >= 0 or free_of[int(E["pre"]["kf_cur"])] >= 0 for E in sc["ie"]]
    return dict(init=init, free=free, free_of=free_of, Kf=Kf, per=per, idx=idx, nb=nb, n=n, included=included, sub=sub, active=active,
                n_active=int(keep.sum()) + sum(active) + (2 if init else 0))


def initial_state(sc):
    st, pts = lc.initial_state(sc)
    shared = dict(bg=np.asarray(sc["bg0"], F64).copy(), ba=np.asarray(sc["ba0"], F64).copy()) if int(sc["init"]) else None
    return st, pts, shared


def _ends(st, shared, a, c):
    """the two ends of an inertial edge as EdgeInertial reads them: the biases are kf_prev's, or the shared pair"""
    O = st[a] if shared is None else dict(st[a], bg=shared["bg"], ba=shared["ba"])
    return st[c], O


def inertial_terms(sc, G, st, shared, variant, jac):
    _, _, nudge, ortho = variant
    out = []
    for m, E in enumerate(sc["ie"]):
        if not G["active"][m]:
            out.append(None)
            continue
        a, c = int(E["pre"]["kf_prev"]), int(E["pre"]["kf_cur"])
        F, O = _ends(st, shared, a, c)
        e, J = pic.inertial_edge(dict(problem=dict(pre=E["pre"])), F, O, nudge, ortho, jac)
        info = lc._iedge_info(E)
        chi = float(e @ (info @ e))
        rho0, rho1 = lc._huber(chi, lc.D_INERTIAL, bool(E["huber"]))
        out.append((e, J, float(rho0), float(rho1), st[c]["bg"] - st[a]["bg"], st[c]["ba"] - st[a]["ba"]))
    return out


def total_cost(sc, G, chi2, terms, shared, order):
    """activeRobustChi2: the visual edges, the inertial edges (with their random walks), the two priors"""
    sub = G["sub"]
    stereo = sub["ur"] >= 0
    rho0, _ = lc._huber(chi2, np.where(stereo, lc.D_STEREO, lc.D_MONO))
    c = float(ordered_sum(rho0, order)) if len(rho0) else 0.0
    for E, t in zip(sc["ie"], terms):
        if t is None:
            continue
        c += t[2]
        if not G["init"]:
            c += float(t[4] @ (E["info_gyro"].reshape(3, 3) @ t[4]))
            c += float(t[5] @ (E["info_acc"].reshape(3, 3) @ t[5]))
    if G["init"]:
        pg, pa = float(F32(sc["prior_g"])), float(F32(sc["prior_a"]))
        ea, eg = 0.0 - shared["ba"], 0.0 - shared["bg"]                         # G2oTypes.h:778-781, :802-805
        c += float(ea @ (pa * ea))
        c += float(eg @ (pg * eg))
    return c


def linearise(sc, G, st, pts, shared, variant):
    """buildSystem -> dict(H [n, n] symmetric, b [n], Hll, bl, W [E, 6, 3], cost)"""
    order = variant[0]
    sub, free_of, idx, Kf, n, nb, init = G["sub"], G["free_of"], G["idx"], G["Kf"], G["n"], G["nb"], G["init"]
    P = len(pts)
    ek, ep = sub["edge_kf"], sub["edge_pt"]
    e, Xc, chi2 = lc.visual_errors(sub, st, pts)
    stereo = sub["ur"] >= 0
    _, rho1 = lc._huber(chi2, np.where(stereo, lc.D_STEREO, lc.D_MONO))
    Ja, Jb = lc.visual_jacobians(sub, st, Xc)
    w = sub["inv"].astype(F64)
    wr = (rho1 * w)[:, None, None]
    omr = (-(w[:, None] * e)) * rho1[:, None]
    Hll = lc._scatter(lc._quad(Ja, wr, Ja), ep, P, order)
    bl = lc._scatter((Ja[:, 0, :] * omr[:, 0, None] + Ja[:, 1, :] * omr[:, 1, None]) + Ja[:, 2, :] * omr[:, 2, None], ep, P, order)
    fe = free_of[ek] if len(ek) else np.zeros(0, np.int64)
    on = fe >= 0
    Hpp = lc._scatter(lc._quad(Jb, wr, Jb)[on], fe[on], Kf, order)
    bp = lc._scatter(((Jb[:, 0, :] * omr[:, 0, None] + Jb[:, 1, :] * omr[:, 1, None]) + Jb[:, 2, :] * omr[:, 2, None])[on], fe[on], Kf, order)
    W = np.where(on[:, None, None], lc._quad(Jb, wr, Ja), 0.0)
    H, b = np.zeros((n, n)), np.zeros(n)
    for i in range(Kf):
        H[6 * i:6 * i + 6, 6 * i:6 * i + 6] = Hpp[i]
        b[6 * i:6 * i + 6] = bp[i]
    terms = inertial_terms(sc, G, st, shared, variant, True)
    seq = range(len(terms)) if order != "reverse" else range(len(terms) - 1, -1, -1)
    for m in seq:
        if terms[m] is None:
            continue
        E = sc["ie"][m]
        ee, J, _, r1, eg, ea = terms[m]
        a, c = int(E["pre"]["kf_prev"]), int(E["pre"]["kf_cur"])
        Hm, bm = pic.quadratic(J, r1 * lc._iedge_info(E), ee, order)
        cols = np.full(24, -1)
        if free_of[a] >= 0:
            cols[0:9] = idx[free_of[a]][:9]
            if not init:
                cols[9:15] = idx[free_of[a]][9:15]
        if init:
            cols[9:15] = nb + np.arange(6)
        if free_of[c] >= 0:
            cols[15:24] = idx[free_of[c]][:9]
        sel = cols >= 0
        H[np.ix_(cols[sel], cols[sel])] += Hm[np.ix_(sel, sel)]
        b[cols[sel]] += bm[sel]
        if init:
            continue
        for info, lo, err in ((E["info_gyro"].reshape(3, 3), 9, eg), (E["info_acc"].reshape(3, 3), 12, ea)):
            Oe = info @ err
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
    if init:                                                                   # linearizeOplus = I (G2oTypes.cc:762-775)
        pg, pa = float(F32(sc["prior_g"])), float(F32(sc["prior_a"]))
        for j in range(3):
            H[nb + j, nb + j] += pg
            H[nb + 3 + j, nb + 3 + j] += pa
        b[nb:nb + 3] += -(pg * (0.0 - shared["bg"]))
        b[nb + 3:nb + 6] += -(pa * (0.0 - shared["ba"]))
    return dict(H=H, b=b, Hll=Hll, bl=bl, W=W, cost=total_cost(sc, G, chi2, terms, shared, order))


def solve_trial(G, L, lam, variant, x_prev):
    """setLambda, the Schur complement over the pose corner, the reduced solve, the points' back substitution"""
    order, solver, _, _ = variant
    sub, free_of, Kf, n = G["sub"], G["free_of"], G["Kf"], G["n"]
    P = len(L["Hll"])
    ek, ep = sub["edge_kf"], sub["edge_pt"]
    D = L["Hll"] + lam * np.eye(3)[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        Dinv = lc._inv3(D) if solver == "ldlt" else (np.linalg.inv(D) if P else D)
    fe = free_of[ek] if len(ek) else np.zeros(0, np.int64)
    on = np.flatnonzero(fe >= 0)
    S = L["H"] + lam * np.eye(n)
    bs = L["b"].copy()
    Wd = np.zeros((P, 6 * Kf, 3))
    for r in range(6):
        Wd[ep[on], 6 * fe[on] + r, :] = L["W"][on, r, :]
    Yd = np.einsum("pak,pkl->pal", Wd, Dinv)
    if P and Kf:
        S[:6 * Kf, :6 * Kf] -= ordered_sum(np.einsum("pak,pbk->pab", Yd, Wd), order)
        bs[:6 * Kf] -= ordered_sum(np.einsum("pak,pk->pa", Yd, L["bl"]), order)
    sol = pic.solve(np.triu(S), bs, solver)
    solved = sol is not None
    x = sol if solved else x_prev
    cl = L["bl"] - np.einsum("pak,a->pk", Wd, x[:6 * Kf]) if Kf else L["bl"]
    return x, np.einsum("pkl,pl->pk", Dinv, cl), solved


def apply_update(sc, G, st, pts, shared, x, xl, variant):
    _, _, nudge, ortho = variant
    new = [dict(s) for s in st]
    for i, k in enumerate(G["free"]):
        K = sc["kf"][k]
        u = np.zeros(15)
        u[:len(G["idx"][i])] = x[G["idx"][i]]
        pic._update(new[k], u, K["Rcb"].reshape(3, 3), K["tcb"], nudge, ortho)
    sh = None if shared is None else dict(bg=shared["bg"] + x[G["nb"]:G["nb"] + 3], ba=shared["ba"] + x[G["nb"] + 3:G["nb"] + 6])
    return new, pts + xl, sh


def optimize(sc, variant=VARIANTS[0], stop_trials=-1, stop_iteration=-1):
    """One call -> dict(status, iterations, trials, rejected_trials, chi2_initial, chi2_final, lambda_final, st, pts [P, 3] (all the
    caller's points), included [P], decision_margin).  stop_trials / stop_iteration: the stop flag is raised once that many trials
    have been made / before that iteration (0 = it is set before optimize())."""
    order = variant[0]
    G = graph(sc)
    st, pts_all, shared = initial_state(sc)
    K = len(sc["kf"])
    out = dict(iterations=0, trials=0, rejected_trials=0, chi2_initial=0.0, chi2_final=0.0, lambda_final=0.0, n_outliers=0, flags=np.zeros(0, bool),
               chi2=np.zeros(0), thr=np.zeros(0), decision_margin=float("inf"), solver_failures=0)
    nothing = K == 0 or (not G["init"] and G["Kf"] == 0)
    if nothing or stop_trials == 0 or stop_iteration == 0:
        return dict(out, status=2 if nothing else 3, st=st, pts=pts_all, included=np.zeros(len(pts_all), bool))
    pts = pts_all[G["included"]]
    n = G["n"]
    lam, ni, n_bad, ok = 0.0, 2.0, 0, G["n_active"] > 0
    iterations = trials = rejected = failures = 0
    dmargin = float("inf")
    x = np.zeros(n)
    chi2_initial = chi2_final = 0.0

    def stopped():
        return (stop_trials >= 0 and trials >= stop_trials) or (stop_iteration >= 0 and iterations >= stop_iteration)
    for it in range(int(sc["iterations"])):
        if stopped() or not ok:                                                # sparse_optimizer.cpp:376
            break
        L = linearise(sc, G, st, pts, shared, variant)
        current = ini = L["cost"]
        if it == 0:
            chi2_initial = current
            lam, ni, n_bad = 1e-5, 2.0, 0                                      # setUserLambdaInit(1e-5), :382
        rho, qmax = 0.0, 0
        while True:
            x, xl, solved = solve_trial(G, L, lam, variant, x)
            st2, pts2, sh2 = apply_update(sc, G, st, pts, shared, x, xl, variant)
            _, _, c2 = lc.visual_errors(G["sub"], st2, pts2)
            temp = total_cost(sc, G, c2, inertial_terms(sc, G, st2, sh2, variant, False), sh2, order)
            if not solved:
                temp = DBL_MAX
                failures += 1
            scale = 0.0
            for i in range(G["Kf"]):
                for j in G["idx"][i]:
                    scale += x[j] * (lam * x[j] + L["b"][j])
            for j in range(G["nb"], n):
                scale += x[j] * (lam * x[j] + L["b"][j])
            scale += float(ordered_sum((xl * (lam * xl + L["bl"])).reshape(-1), "forward")) if len(pts) else 0.0
            rho = (current - temp) / (scale + 1e-3)
            trials += 1
            dmargin = min(dmargin, abs(current - temp) / max(current, 1.0))
            if rho > 0 and math.isfinite(temp):
                y = 2 * rho - 1
                lam *= max(1.0 / 3.0, min(1.0 - (y * y) * y, 2.0 / 3.0))
                ni = 2.0
                current = temp
                st, pts, shared = st2, pts2, sh2
            else:
                lam *= ni
                ni *= 2
                rejected += 1
            qmax += 1
            if not (rho < 0 and qmax < 10 and not stopped()):                  # levenberg.cpp:149
                break
        iterations += 1
        chi2_final = current
        if qmax == 10 or rho == 0:
            ok = False
            continue
        n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
        if n_bad >= 3:
            ok = False
    if iterations == 0:
        chi2_final = chi2_initial
    if shared is not None:                                                     # :720-733: every KeyFrame with bImu receives the shared pair
        st = [dict(s, bg=shared["bg"], ba=shared["ba"]) if sc["kf"]["kind"][k] != 2 else s for k, s in enumerate(st)]
    pts_all = pts_all.copy()
    pts_all[G["included"]] = pts
    return dict(out, status=0, iterations=iterations, trials=trials, rejected_trials=rejected, chi2_initial=chi2_initial, chi2_final=chi2_final,
                lambda_final=lam, st=st, pts=pts_all, included=G["included"], decision_margin=dmargin, solver_failures=failures)


# ------------------------------------------------------------------------------------------------ scenes
def build(seed, n_kf, n_points, init=0, iterations=3, fixed=(), cut=(), far=0, priors=PRIORS[1], bias0=1.0, stop_trials=-1, stop_iteration=-1, **kw):
    """A map of n_kf KeyFrames along one inertial chain (local_inertial_ba_cases.build's generator), every one of them with inertial
    vertices.  fixed: the KeyFrames that are fixed (kind 1), the others are free, the first of the chain included; cut: inertial
    edges left out (the KeyFrame after one has no incoming edge: two chains); far: points added that are seen by one of the first
    six and one of the last six KeyFrames only; bias0: the shared pair starts at bias0 times the last KeyFrame's biases (InitializeIMU
    starts it near zero, and EdgePriorAcc's weight of 1e10 leaves a start far from zero no trial that gains)."""
    sc = lc.build(seed, n_kf - 1, n_points, n_fixed=0, iterations=iterations, **kw)
    rng = np.random.default_rng(seed + 700001)
    kf = sc["kf"].copy()
    start = kw.get("start", 1.0)
    t = sc["truth"][0]                                                         # the chain's first KeyFrame starts away from the truth as the others do
    lc._kf_record(kf[0], pic._f32(t["Rwb"] @ _rot(start * rng.normal(0, 0.004, 3))), pic._f32(t["twb"] + start * rng.normal(0, 0.01, 3)),
                  pic._f32(t["v"] + start * rng.normal(0, 0.02, 3)), pic._f32(t["bg"] + rng.normal(0, 3e-4, 3)),
                  pic._f32(t["ba"] + rng.normal(0, 3e-3, 3)), 0)
    kf["kind"] = 0
    kf["kind"][list(fixed)] = 1
    ie = sc["ie"].copy()
    ie["huber"], ie["downweight"] = 1, 0                                       # :499-501; no information() * 1e-2
    links = [m for m in range(len(ie)) if m not in cut]
    ie, c15 = ie[links], sc["C15"][links]
    octave = sc["octave"]
    pos, ek, ep, xy, ur, inv = (sc[k] for k in ("pos", "edge_kf", "edge_pt", "xy", "ur", "inv"))
    if far:
        cams = [(pic.RCB @ q["Rwb"].T, pic.RCB @ (-q["Rwb"].T @ q["twb"]) + pic.TCB) for q in sc["truth"]]
        npos, nek, nep, nxy, nur, ninv = [], [], [], [], [], []
        for j in range(far):
            a, b = int(rng.integers(0, 6)) + (1 if 0 in fixed else 0), int(n_kf - 6 + rng.integers(0, 6))
            Xc = np.array([rng.uniform(-30, 30), rng.uniform(-8, 8), rng.uniform(150, 300)])
            Xw = cams[a][0].T @ (Xc - cams[a][1])
            for k in (a, b):
                Xk = cams[k][0] @ Xw + cams[k][1]
                assert Xk[2] > 50
                nek.append(k)
                nep.append(len(pos) + j)
                nxy.append([pic.KITTI["fx"] * Xk[0] / Xk[2] + pic.KITTI["cx"] + 0.6 * rng.normal(), pic.KITTI["fy"] * Xk[1] / Xk[2] + pic.KITTI["cy"] + 0.6 * rng.normal()])
                nur.append(-1.0)
                ninv.append(1.0)
            npos.append(Xw + rng.normal(0, 1.0, 3))
        pos = np.concatenate([pos, np.asarray(npos, F32)])
        ek, ep = np.concatenate([ek, np.asarray(nek, np.int32)]), np.concatenate([ep, np.asarray(nep, np.int32)])
        octave = np.concatenate([octave, np.zeros(len(nek), np.int32)])
        xy, ur, inv = np.concatenate([xy, np.asarray(nxy, F32)]), np.concatenate([ur, np.asarray(nur, F32)]), np.concatenate([inv, np.asarray(ninv, F32)])
    last = kf[-1]
    return dict(init=int(init), iterations=int(iterations), prior_g=F32(priors[0]), prior_a=F32(priors[1]), bg0=bias0 * last["bg"], ba0=bias0 * last["ba"],
                kf=kf, ie=ie, pos=pos, edge_kf=ek, edge_pt=ep, xy=xy, ur=ur, inv=inv, planted=sc["planted"], depth=sc["depth"], speed=sc["speed"],
                stop_trials=stop_trials, stop_iteration=stop_iteration, truth=sc["truth"], C15=c15, octave=octave)


# name -> (seed, KeyFrames, points, keywords).  The cost has steps of about 1e-7 of its value (the preintegration's bias correction is
# float32), so the scenes stop before Levenberg has converged to that floor (decision_margin, checked by the CPU test).
_SCENES = {
    # init = 0: n = 15 Kf against the 48-wide panel of the blocked solve.  The larger maps have one fixed KeyFrame: without one the
    # four gauge directions are held by lambda = 1e-5 alone and D grows with the size of the map (see measure()).
    "f1": (401, 2, 30, dict(iterations=3, fixed=(0,), start=3.0)),
    "f3": (402, 3, 40, dict(iterations=3)),
    "f4": (403, 4, 40, dict(iterations=3)),
    "f16": (404, 17, 80, dict(iterations=3, fixed=(0,), start=3.0)),
    "f26": (405, 27, 100, dict(iterations=3, fixed=(0,), start=3.0)),
    "f40_far": (406, 41, 120, dict(iterations=3, far=40, fixed=(0,), start=3.0)),
    # init = 1: n = 9 Kf + 6
    "i1": (411, 2, 30, dict(init=1, iterations=3, fixed=(0,), start=3.0)),
    "i5": (412, 6, 40, dict(init=1, iterations=3, priors=PRIORS[0], bias0=1e-3, fixed=(0,), start=3.0)),
    "i10": (413, 10, 60, dict(init=1, iterations=3)),
    "j27": (454, 27, 100, dict(init=1, iterations=2, priors=PRIORS[2], start=3.0)),                      # 27 KeyFrames, none fixed
    "i27": (414, 28, 100, dict(init=1, iterations=3, priors=PRIORS[2], fixed=(0,), start=3.0)),
    # fixed KeyFrames, two of them adjacent: the inertial edge between them is active only with init
    "f_fixed": (421, 8, 60, dict(iterations=3, fixed=(0, 3, 4), start=3.0)),
    "i_fixed": (422, 8, 60, dict(init=1, iterations=3, fixed=(0, 3, 4), start=3.0)),
    "mono_only": (431, 4, 60, dict(iterations=3, mono_frac=1.0)),
    "stereo_only": (432, 4, 40, dict(iterations=3, mono_frac=0.0)),
    "mixed": (433, 4, 40, dict(init=1, iterations=3, mono_frac=0.5)),
    "e1025": (434, 6, 400, dict(iterations=3, max_edges=1031, fixed=(0,), start=3.0)),   # 1025 of them end at a vertex
    "p257": (445, 4, 272, dict(init=1, iterations=3, obs_frac=0.5, fixed=(0,), start=3.0)),       # 257 of them are vertices
    "fixed_only_point": (436, 6, 40, dict(iterations=3, fixed=(0, 1), fixed_only=5, start=3.0)),
    "outliers": (437, 5, 80, dict(iterations=5, outliers=0.2, start=10.0)),
    "rejected_trials": (444, 6, 60, dict(iterations=6, outliers=0.15, start=30.0)),
    "it1": (439, 3, 40, dict(iterations=1)),
    "it7": (440, 6, 60, dict(iterations=7, outliers=0.15, start=30.0)),
    "two_chains": (441, 7, 60, dict(iterations=3, cut=(3,))),
    "i_two_chains": (442, 8, 60, dict(init=1, iterations=3, cut=(3,), priors=PRIORS[0], bias0=1e-3, fixed=(0,), start=3.0)),
    # the stop flag: raised once five trials have been made, which is after a rejected trial of the third iteration; raised before
    # iteration 2
    "stop_trial": (403, 4, 40, dict(iterations=3, stop_trials=5)),
    "stop_iteration": (404, 17, 80, dict(iterations=5, fixed=(0,), start=3.0, stop_iteration=2)),
}
ALL = tuple(_SCENES)
# Free-gauge maps of the init = 0 form at 16 KeyFrames and more.  They are NOT scenes of the comparison: the restatement's own variants
# disagree on them by more than a sixteenth of what the vertices move (g16: 0.04 on an entry of Rwb that moves 0.1) or in their
# decisions (g40_far: three failed factorisations in the forward variant, other counts in others), because lambda = 1e-5 alone holds
# the four gauge directions.  The CPU test pins that finding; the GPU test runs them for what can be asked there.
_LIMIT_SCENES = {
    "g16": (451, 16, 80, dict(iterations=2)),
    "g26": (452, 26, 100, dict(iterations=2)),
    "g40_far": (453, 40, 120, dict(iterations=2, far=40)),
}
LIMIT = tuple(_LIMIT_SCENES)
NO_FIXED = tuple(n for n in ALL if not _SCENES[n][3].get("fixed")) + LIMIT


@functools.lru_cache(maxsize=None)
def scene(name):
    seed, n_kf, n_points, kw = _SCENES[name] if name in _SCENES else _LIMIT_SCENES[name]
    sc = build(seed, n_kf, n_points, **dict(kw))
    if name == "fixed_only_point":                                             # ... and a point without an edge
        sc = dict(sc, pos=np.concatenate([sc["pos"], np.asarray([[1.0, 2.0, 3.0]], F32)]))
    return sc


@functools.lru_cache(maxsize=None)
def reference(name, variant=VARIANTS[0]):
    sc = scene(name)
    return optimize(sc, variant, sc["stop_trials"], sc["stop_iteration"])


# ------------------------------------------------------------------------------------------------ comparison
def differences(a, b, sc):
    d = lc.differences(a, b, sc)
    return {k: d[k] for k in QUANTITIES}


def decisions(r):
    """what must be equal between any two statements of the routine"""
    return (int(r["status"]), int(r["iterations"]), int(r["trials"]), int(r["rejected_trials"]), tuple(bool(f) for f in r["included"]),
            int(r["solver_failures"]))


def movement(sc, r):
    """how far the free vertices moved from their start, per quantity in the units of differences(): the smallest over the free
    KeyFrames (init: over the shared pair for bg, ba) and over the included points"""
    st0, pts0, shared0 = initial_state(sc)
    free = np.flatnonzero(sc["kf"]["kind"] == 0)
    scale = dict(Rwb=1.0, twb=sc["depth"], v=max(sc["speed"], 1e-3), bg=1.0, ba=1.0)
    m = {}
    for q, u in scale.items():
        if shared0 is not None and q in ("bg", "ba"):
            k = int(np.flatnonzero(sc["kf"]["kind"] != 2)[0])
            m[q] = float(np.abs(r["st"][k][q] - shared0[q]).max())
        else:
            m[q] = min([float(np.abs(r["st"][k][q] - st0[k][q]).max() / u) for k in free] + [float("inf")])
    inc = np.asarray(r["included"], bool)
    m["points"] = float((np.abs(r["pts"] - pts0).max(axis=1) / sc["depth"])[inc].min()) if inc.any() else float("inf")
    return m


def from_records(rec, kf_out, pos_d, included):
    st = [dict(Rwb=k["Rwb"].reshape(3, 3), twb=k["twb"], v=k["v"], bg=k["bg"], ba=k["ba"], Rcw=k["Rcw"].reshape(3, 3), tcw=k["tcw"]) for k in kf_out]
    return dict(status=int(rec["status"]), iterations=int(rec["iterations"]), trials=int(rec["trials"]), rejected_trials=int(rec["rejected_trials"]),
                chi2_initial=float(rec["chi2_initial"]), chi2_final=float(rec["chi2_final"]), lambda_final=float(rec["lambda_final"]), st=st,
                pts=np.asarray(pos_d, F64).reshape(-1, 3), included=np.asarray(included, bool), chi2=np.zeros(0), thr=np.zeros(0),
                solver_failures=int(rec["reserved"]))


def problem_record(sc):
    p = np.zeros(1, FIBA_PROBLEM_DTYPE)
    for k in ("init", "iterations", "prior_g", "prior_a", "bg0", "ba0"):
        p[k] = sc[k]
    return p


def write_scenes(path, scenes):
    with open(path, "wb") as f:
        f.write(np.int32(len(scenes)).tobytes())
        for sc in scenes:
            f.write(np.array([sc["init"], sc["iterations"], len(sc["kf"]), len(sc["ie"]), len(sc["pos"]), len(sc["edge_kf"]), sc["stop_trials"],
                              sc["stop_iteration"]], np.int32).tobytes())
            f.write(problem_record(sc).tobytes()[8:])
            for k, dt in (("kf", lc.KF_DTYPE), ("ie", lc.IEDGE_DTYPE), ("pos", F32), ("edge_kf", np.int32), ("edge_pt", np.int32), ("xy", F32),
                          ("ur", F32), ("inv", F32)):
                f.write(np.ascontiguousarray(sc[k], dt).tobytes())


def read_results(path, scenes):
    out = []
    with open(path, "rb") as f:
        for sc in scenes:
            K, P = len(sc["kf"]), len(sc["pos"])
            rec = np.frombuffer(f.read(lc.RESULT_DTYPE.itemsize), lc.RESULT_DTYPE)[0]
            ko = np.frombuffer(f.read(K * lc.KF_OUT_DTYPE.itemsize), lc.KF_OUT_DTYPE)
            pts = np.frombuffer(f.read(24 * P), F64)
            inc = np.frombuffer(f.read(P), np.uint8)
            out.append((rec, ko, from_records(rec, ko, pts, inc)))
        assert f.read() == b""
    return out


def write_dropin_scene(path, sc, loop_id):
    """what tests/dropin_full_inertial_ba_main.cc builds its stand-in map from: write_scenes' records plus every edge's 15 x 15
    covariance, the octaves and mvInvLevelSigma2"""
    assert np.array_equal(pic.LEVEL_INV_SIGMA2[sc["octave"]], sc["inv"]) and (sc["kf"]["kind"] == 0).all()
    with open(path, "wb") as f:
        f.write(np.array([sc["init"], sc["iterations"], loop_id, len(sc["kf"]), len(sc["ie"]), len(sc["pos"]), len(sc["edge_kf"])], np.int32).tobytes())
        f.write(np.array([sc["prior_g"], sc["prior_a"]], F32).tobytes())
        for k, dt in (("kf", lc.KF_DTYPE), ("ie", lc.IEDGE_DTYPE), ("C15", F32), ("pos", F32), ("edge_kf", np.int32), ("edge_pt", np.int32), ("xy", F32),
                      ("ur", F32), ("octave", np.int32)):
            f.write(np.ascontiguousarray(sc[k], dt).tobytes())
        f.write(pic.LEVEL_INV_SIGMA2.tobytes())


def read_scenes(f):
    """write_scenes' layout back -> a list of scene dicts"""
    out = []
    for _ in range(int(np.frombuffer(f.read(4), np.int32)[0])):
        init, its, K, NI, P, E, st, si = (int(v) for v in np.frombuffer(f.read(32), np.int32))
        pg, pa = np.frombuffer(f.read(8), F32)
        b = np.frombuffer(f.read(48), F64)
        sc = dict(init=init, iterations=its, stop_trials=st, stop_iteration=si, prior_g=pg, prior_a=pa, bg0=b[:3].copy(), ba0=b[3:].copy())
        sc["kf"] = np.frombuffer(f.read(K * lc.KF_DTYPE.itemsize), lc.KF_DTYPE)
        sc["ie"] = np.frombuffer(f.read(NI * lc.IEDGE_DTYPE.itemsize), lc.IEDGE_DTYPE)
        sc["pos"] = np.frombuffer(f.read(12 * P), F32).reshape(-1, 3)
        sc["edge_kf"], sc["edge_pt"] = np.frombuffer(f.read(4 * E), np.int32), np.frombuffer(f.read(4 * E), np.int32)
        sc["xy"] = np.frombuffer(f.read(8 * E), F32).reshape(-1, 2)
        sc["ur"], sc["inv"] = np.frombuffer(f.read(4 * E), F32), np.frombuffer(f.read(4 * E), F32)
        out.append(sc)
    return out


DROPIN_KF = np.dtype([("n_set_pose", "<i4"), ("n_set_velocity", "<i4"), ("n_set_bias", "<i4"), ("gba_mark", "<i4"), ("Rcw", "<f4", 9), ("tcw", "<f4", 3),
                      ("v", "<f4", 3), ("bias", "<f4", 6), ("Rcw_gba", "<f4", 9), ("tcw_gba", "<f4", 3), ("v_gba", "<f4", 3), ("bias_gba", "<f4", 6)])
DROPIN_PT = np.dtype([("n_set_pos", "<i4"), ("n_update", "<i4"), ("gba_mark", "<i4"), ("pos", "<f4", 3), ("pos_gba", "<f4", 3)])


def read_dropin_result(path, sc):
    """-> (the gathered problem as a scene dict, dict(ret, change, n_new_bias, kf [K] records, pts [P] records))"""
    with open(path, "rb") as f:
        g = read_scenes(f)[0]
        ret, change, n_new_bias = np.frombuffer(f.read(12), np.int32)
        kf = np.frombuffer(f.read(len(sc["kf"]) * DROPIN_KF.itemsize), DROPIN_KF)
        pts = np.frombuffer(f.read(len(sc["pos"]) * DROPIN_PT.itemsize), DROPIN_PT)
        assert f.read() == b""
    return g, dict(ret=int(ret), change=int(change), n_new_bias=int(n_new_bias), kf=kf, pts=pts)


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def bounds(name):
    """16 D of the scene's own group (with / without a fixed KeyFrame): never wider than 16 times the D over all scenes"""
    return {k: MARGIN * v for k, v in golden()["D_no_fixed" if name in NO_FIXED else "D_fixed"].items()}


def within(d, b):
    return all(d[k] <= b[k] for k in d if k in b)


def measure(names=ALL):
    """D per quantity over the scenes and the variants, for all scenes and for those with / without a fixed KeyFrame apart, and
    per scene its decisions, its movement, its decision margin and its own D"""
    D, Dn, Df = ({k: 0.0 for k in QUANTITIES} for _ in range(3))
    agree, per_scene = True, {}
    for nm in names:
        sc = scene(nm)
        base = reference(nm)
        own = {}
        for var in VARIANTS[1:]:
            r = optimize(sc, var, sc["stop_trials"], sc["stop_iteration"])
            if decisions(r) != decisions(base):
                agree = False
                print("decisions differ:", nm, var)
                continue
            for k, v in differences(base, r, sc).items():
                own[k] = max(own.get(k, 0.0), v)
        for k, v in own.items():
            D[k] = max(D[k], v)
            part = Dn if nm in NO_FIXED else Df
            part[k] = max(part[k], v)
        per_scene[nm] = dict(decisions=list(decisions(base)[:4]), movement=movement(sc, base), decision_margin=min(base["decision_margin"], 1e300), D=own)
    return dict(D=D, D_no_fixed=Dn, D_fixed=Df, variants_agree=agree, margin=MARGIN, variants=[list(v) for v in VARIANTS], scenes=per_scene)


if __name__ == "__main__":
    if "--measure" in sys.argv:
        m = measure()
        with open(GOLDEN, "w") as f:
            json.dump(m, f, indent=1, sort_keys=True)
        print(json.dumps(m, indent=1, sort_keys=True))
