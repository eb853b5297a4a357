"""The welding bundle adjustment of a visual map merge, the second Optimizer::LocalBundleAdjustment (pMainKF, vpAdjustKF,
vpFixedKF, pbStopFlag; src/Optimizer.cc:3494-3915, pinhole KeyFrames) after its gathering loops, restated in float64 numpy on the
pieces of tests/local_ba_cases.py, which are imported unchanged: the edges, the plan, the ordered sums, the Levenberg loop
(levenberg), the L D L^T, the scene generator.  Also the named scenes of the GPU tests.  No GPU, no library.

`python tests/welding_ba_cases.py --measure` writes tests/golden/welding_ba_sensitivity.json.

What the routine does that LocalBundleAdjustment and BundleAdjustment do not, it optimises TWICE over TWO graphs:
  * optimize(5) with Huber kernels on every edge, (float)sqrt(5.99) wide for mono (:3607, the global BA's width) and
    (float)sqrt(7.815) for stereo;
  * :3726-3753: an edge with chi2() > 5.991 / 7.815 (compared in DOUBLE: nothing narrows here) or !isDepthPositive() goes to level
    1; every kernel is switched off.  There is NO computeError() before it, so chi2() is what the last computeActiveErrors() left:
    the errors at the state of the last TRIAL, which pop() has discarded if that trial was rejected.  isDepthPositive() reads the
    vertices: the accepted state;
  * initializeOptimization(0) + optimize(10): the level-0 edges only.  A vertex no level-0 edge reaches is not in the problem: here
    the edges are compacted, and a free KeyFrame that lost all of its edges is handed to levenberg as a fixed one.  A point without
    an active edge stays in the arrays with an empty run, which adds +0.0 to it and 0 to computeLambdaInit and computeScale.
    levenberg starts lambda, ni and the bad-iteration count anew, as g2o's iteration 0 does;
  * :3769-3803: the same test, again without computeError(): an edge of round 2 has the chi2 of round 2's last trial (when round 2
    made no iteration, what round 1 left), a level-1 edge that of round 1's last trial; the depth is read at the final state;
  * the flag: set on entry -> status 2, nothing touched (:3709-3711); up after round 1 -> status 3, no levels, no round 2, the one
    classification (:3716-3760).

`variant`: the summation orders and the elimination of local_ba_cases (forward = g2o's order, THE REFERENCE VALUE).
`chi2_at="accepted"` is a WRONG statement kept for tests/test_welding_ba_cpu.py: it classifies with the errors at the accepted
state, as LocalBundleAdjustment's computeError() would.  The two differ only when a round ends on a rejected trial.  Without the
stop flag that takes ten rejections in a row (levenberg.cpp:149), after which the two states agree to 1e-9; with it, any rejected
trial will do.  So the scenes of STOP_SCENES raise the flag at a chosen poll (STOPS), here through levenberg below and in the
library through msorb_debug_welding_ba_poll_hook, which calls the test before every read of the flag."""
import json
import math
import os
import sys
import time

import numpy as np

import local_ba_cases as lc
import pose_opt_cases as pc
from local_ba_cases import VARIANTS, CHI2_MONO, CHI2_STEREO, estimate_distance
from pose_opt_cases import F32, F64, normalize_rotation

DELTA_MONO = float(F32(math.sqrt(5.99)))      # Optimizer.cc:3607
DELTA_STEREO = pc.DELTA_STEREO                # :3608
ROUND_KEYS = ("iterations", "trials", "rejected_trials")


class Recording(lc.Problem):
    """a Problem that remembers the chi2 of its last error() call: what e->chi2() returns until the next computeActiveErrors()"""
    last_chi2 = None

    def error(self, q, t, X):
        e, p, chi2 = super().error(q, t, X)
        self.last_chi2 = chi2
        return e, p, chi2


def no_kernel(chi2):
    return chi2, np.ones_like(chi2)            # setRobustKernel(0): rho = chi2, weight 1


def chi2_flags(chi2, stereo):
    """chi2() > 5.991 / 7.815 in double (:3733, :3747, :3776, :3794); a NaN is not greater"""
    with np.errstate(all="ignore"):
        return np.asarray(chi2, F64) > np.where(stereo, CHI2_STEREO, CHI2_MONO)


def classify(chi2_flag, depth):
    """the test of both classifications from its two parts: the chi2 flag an edge carries and the depth at the estimate"""
    with np.errstate(all="ignore"):
        return np.asarray(chi2_flag, bool) | ~(np.asarray(depth, F64) > 0.0)


# where the stop flag is read after the entry check (MSORB_WELDING_POLL_*): before an iteration (sparse_optimizer.cpp:376), after a
# rejected trial whose rho is negative (levenberg.cpp:149), between the rounds (Optimizer.cc:3718)
POLL_ITERATION, POLL_REJECTED, POLL_BETWEEN = 0, 1, 2
# name -> when the flag rises: f(round, where, iteration, trials of the round so far); the library's poll hook raises it at the same poll
STOPS = {
    "between": lambda rnd, where, it, trials: where == POLL_BETWEEN,
    "round1_rejected": lambda rnd, where, it, trials: rnd == 0 and where == POLL_REJECTED,      # right after round 1's first rejected trial
    "round1_it2": lambda rnd, where, it, trials: rnd == 0 and where == POLL_ITERATION and it == 2,
    "round2_it3": lambda rnd, where, it, trials: rnd == 1 and where == POLL_ITERATION and it == 3,
    "round2_first": lambda rnd, where, it, trials: rnd == 1,                                    # before round 2's first iteration
}


def levenberg(pr, q, t, X, variant, iterations, huber, poll):
    """local_ba_cases.levenberg with terminate() at its two places: poll(where, iteration, trials) -> the flag is up.  Line for line
    lc.levenberg otherwise (tests/test_welding_ba_cpu.py holds the two against each other with a flag that stays down)."""
    order = lc._order(variant)
    pl = pr.plan
    P, E, Kf = pr.P, pr.E, pl.Kf
    res = dict(iterations=0, trials=0, rejected_trials=0, chi2_initial=0.0, chi2_final=0.0)
    n = 6 * Kf
    x = np.zeros(n + 3 * P, F64)
    lam, ni, n_bad, ok = 0.0, 2.0, 0, E > 0
    it = 0
    while it < iterations and not poll(POLL_ITERATION, it, res["trials"]) and ok:      # sparse_optimizer.cpp:376
        e, p, chi2 = pr.error(q, t, X)
        rho0, rho1 = huber(chi2)
        current = float(lc.ordered_sum(rho0[:, None], order)[0])
        ini = current
        Ja, Jb = pr.jacobians(q, p)
        eHll, ebl, eHpp, ebp, W = pr.quadratic_forms(e, rho1, Ja, Jb)
        Hl = lc.seg_sum(np.concatenate([eHll, ebl], 1), pr.ep, P, order)
        Hll, bl = Hl[:, :6], Hl[:, 6:]
        Hp = lc.seg_sum(np.concatenate([eHpp, ebp], 1)[pl.kf_edge], pl.kf_seg, Kf, order)
        Hpp, bp = Hp[:, :21], Hp[:, 21:]
        if it == 0:
            res["chi2_initial"] = current
            diag = np.concatenate([np.abs(Hpp[:, [0, 6, 11, 15, 18, 20]]).ravel(), np.abs(Hll[:, [0, 3, 5]]).ravel()])
            lam, ni, n_bad = 1e-5 * float(max(diag.max() if len(diag) else 0.0, 0.0)), 2.0, 0
        rho, qmax = 0.0, 0
        while True:
            bq, bt, bX = q.copy(), t.copy(), X.copy()
            if variant == "dense":
                ok2 = lc._solve_dense(pr, Hpp, bp, Hll, bl, W, lam, x)
            else:
                ok2 = lc._solve_schur(pr, Hpp, bp, Hll, bl, W, lam, x, order, lc.ldlt_solve)
            for i in range(Kf):
                k = pl.kf_of_free[i]
                nq, nt = lc.oplus(list(q[k]), list(t[k]), [float(v) for v in x[6 * i:6 * i + 6]])
                q[k], t[k] = nq, nt
            X = X + x[n:].reshape(P, 3)
            _, _, chi2 = pr.error(q, t, X)
            r0, _ = huber(chi2)
            temp = float(lc.ordered_sum(r0[:, None], order)[0])
            if not ok2:
                temp = lc.DBL_MAX
            b_all = np.concatenate([bp.ravel(), bl.ravel()])
            with np.errstate(all="ignore"):
                scale = float(lc.ordered_sum((x * (lam * x + b_all))[:, None], order)[0]) + 1e-3
                rho = float((F64(current) - F64(temp)) / F64(scale))
            res["trials"] += 1
            if rho > 0 and math.isfinite(temp):
                yy = 2 * rho - 1
                alpha = min(1. - (yy * yy) * yy, 2. / 3.)
                lam *= max(1. / 3., alpha)
                ni = 2.0
                current = temp
            else:
                lam *= ni
                ni *= 2
                q, t, X = bq, bt, bX
                res["rejected_trials"] += 1
            qmax += 1
            if not (rho < 0 and qmax < 10 and not poll(POLL_REJECTED, it, res["trials"])):     # levenberg.cpp:149
                break
        res["iterations"] += 1
        res["chi2_final"] = current
        it += 1
        if qmax == 10 or rho == 0:
            ok = False
            continue
        if (ini - current) * 1e3 < ini:
            n_bad += 1
        else:
            n_bad = 0
        if n_bad >= 3:
            ok = False
    if res["iterations"] == 0:
        res["chi2_final"] = res["chi2_initial"]
    return q, t, X, lam, res


def _with_fixed(kf, fixed):
    if isinstance(kf, dict):
        return dict(kf, fixed=np.asarray(fixed, np.int32))
    out = kf.copy()
    out["fixed"] = fixed
    return out


def second_graph(s, level1):
    """initializeOptimization(0) (sparse_optimizer.cpp:199-260): the level-0 edges, and as fixed every KeyFrame none of them reaches
    -> (scene of round 2, active edge indices, active free KeyFrames [K] bool, active points [P] bool)"""
    fixed = np.asarray(s["kf"]["fixed"]).astype(bool)
    act = np.nonzero(~np.asarray(level1, bool))[0]
    ek, ep = np.asarray(s["edge_kf"], int)[act], np.asarray(s["edge_point"], int)[act]
    kf_active = np.zeros(len(fixed), bool)
    kf_active[ek] = True
    kf_active &= ~fixed
    pt_active = np.zeros(len(s["pos_w"]), bool)
    pt_active[ep] = True
    sub = dict(kf=_with_fixed(s["kf"], (~kf_active).astype(np.int32)), pos_w=s["pos_w"], edge_kf=ek, edge_point=ep,
               xy=np.asarray(s["xy"]).reshape(-1, 2)[act], u_right=np.asarray(s["u_right"])[act], inv_sigma2=np.asarray(s["inv_sigma2"])[act])
    return sub, act, kf_active, pt_active


def welding_ba(s, variant="forward", stop=None, chi2_at="trial"):
    """s: a scene (kf, pos_w, edge_kf, edge_point, xy, u_right, inv_sigma2).  stop: None, "before" (the flag is set on entry), a
    name of STOPS, or a function like theirs (the flag rises at that poll and stays up).
    -> dict(status, round [2 x dict(iterations, trials, rejected_trials, chi2_initial, chi2_final, lambda_final)], level1 [E],
    outlier [E], n_level1, n_outliers, active_keyframes, active_points, kf_qt_d [K, 7], kf_qt, pos_d [P, 3], pos, and for the tests:
    round1_kf_qt_d, round1_pos_d (the state round 1 left), chi2_flag1 / depth1 (the two parts of the first classification),
    chi2_trial1, kf_active, pt_active)"""
    assert chi2_at in ("trial", "accepted")
    rises = STOPS.get(stop, stop) if stop not in (None, "before") else None
    up = [False]                                                  # the stop flag: once up it stays up

    def poll(rnd, where, it, trials):
        up[0] = up[0] or bool(rises and rises(rnd, where, it, trials))
        return up[0]

    def optimize(problem, q, t, X, iterations, huber, rnd):
        if rises is None:
            return lc.levenberg(problem, q, t, X, variant, iterations, huber)
        return levenberg(problem, q, t, X, variant, iterations, huber, lambda where, it, trials: poll(rnd, where, it, trials))

    pr = Recording(s)
    pr.delta = np.where(pr.stereo, DELTA_STEREO, DELTA_MONO)
    K, P, E = pr.K, pr.P, pr.E
    kf = s["kf"]
    q_in, t_in, X_in = np.asarray(kf["q"]), np.asarray(kf["t"]), np.asarray(s["pos_w"])
    zero_round = dict(iterations=0, trials=0, rejected_trials=0, chi2_initial=0.0, chi2_final=0.0, lambda_final=0.0)
    res = dict(status=0, round=[dict(zero_round), dict(zero_round)], level1=np.zeros(E, bool), outlier=np.zeros(E, bool), n_level1=0,
               n_outliers=0, active_keyframes=0, active_points=0)

    def finish(q, t, X):
        qt = np.concatenate([q, t], 1)
        qt[pr.fixed] = np.concatenate([q_in, t_in], 1).astype(F64)[pr.fixed]      # a fixed KeyFrame's output repeats its input
        res.update(kf_qt_d=qt, pos_d=X, kf_qt=qt.astype(F32), pos=X.astype(F32))   # :3908, :3912
        return res

    if stop == "before":                                          # :3709-3711
        res["status"] = 2
        res.update(kf_qt_d=np.concatenate([q_in, t_in], 1).astype(F64), pos_d=X_in.astype(F64))
        res["kf_qt"], res["pos"] = res["kf_qt_d"].astype(F32), res["pos_d"].astype(F32)
        return res
    q = np.array([normalize_rotation(v) for v in q_in.astype(F64)]).reshape(-1, 4)      # SE3Quat's constructor normalises
    t = t_in.astype(F64).copy()
    X = X_in.astype(F64).copy()

    def chi2_after(problem, counts, q, t, X, before):
        """what chi2() returns after an optimize(): the last trial's errors; `before` where no error was computed"""
        if counts["iterations"] == 0:
            return before
        return problem.last_chi2.copy() if chi2_at == "trial" else problem.error(q, t, X)[2]

    # ---- round 1, :3713-3714 ----
    q, t, X, lam, c = optimize(pr, q, t, X, 5, pr.huber, 0)
    if E > 0 and c["iterations"] == 0:                            # the flag rose before the first iteration: as the early return
        res["status"] = 2
        res.update(kf_qt_d=np.concatenate([q_in, t_in], 1).astype(F64), pos_d=X_in.astype(F64))
        res["kf_qt"], res["pos"] = res["kf_qt_d"].astype(F32), res["pos_d"].astype(F32)
        return res
    res["round"][0] = dict(c, lambda_final=lam)
    chi2 = chi2_after(pr, c, q, t, X, np.zeros(E))
    flag = chi2_flags(chi2, pr.stereo)
    depth = pr.error(q, t, X)[1][:, 2]
    res.update(round1_kf_qt_d=np.concatenate([q, t], 1).copy(), round1_pos_d=X.copy(), chi2_flag1=flag.copy(), depth1=depth.copy(),
               chi2_trial1=np.asarray(chi2).copy(), kf_active=np.zeros(K, bool), pt_active=np.zeros(P, bool))
    if poll(0, POLL_BETWEEN, c["iterations"], c["trials"]):       # :3716-3721: bDoMore = false
        res["status"] = 3
    else:
        # ---- :3726-3753 ----
        level1 = classify(flag, depth)
        res.update(level1=level1, n_level1=int(level1.sum()))
        # ---- round 2, :3758-3759 ----
        sub, act, kf_active, pt_active = second_graph(s, level1)
        pr2 = Recording(sub)
        q, t, X, lam, c = optimize(pr2, q, t, X, 10, no_kernel, 1)
        res["round"][1] = dict(c, lambda_final=lam)
        res.update(active_keyframes=int(kf_active.sum()), active_points=int(pt_active.sum()), kf_active=kf_active, pt_active=pt_active)
        flag = flag.copy()
        flag[act] = chi2_flags(chi2_after(pr2, c, q, t, X, chi2[act]), pr2.stereo)       # a level-1 edge keeps round 1's
    # ---- :3769-3803 ----
    depth = pr.error(q, t, X)[1][:, 2]
    outlier = classify(flag, depth)
    res.update(outlier=outlier, n_outliers=int(outlier.sum()), chi2_flag=flag, depth=depth)
    return finish(q, t, X)


# ---------------------------------------------------------------------------------------------------------------- scenes
def _gross(s, edges, rng, lo=60.0, hi=200.0):
    """a gross error of lo-hi px on the named edges"""
    xy = np.asarray(s["xy"]).copy()
    for e in edges:
        a, m = rng.uniform(0, 2 * math.pi), rng.uniform(lo, hi)
        xy[e] += np.array([math.cos(a), math.sin(a)], xy.dtype) * xy.dtype.type(m)
    s["xy"] = xy


def _keep_edges(s, keep):
    for k in ("edge_kf", "edge_point", "xy", "u_right", "inv_sigma2", "planted"):
        s[k] = np.asarray(s[k])[keep]


def make_scene(seed, drop_kf=None, drop_kf_edges=4, drop_point=None, extra_point=False, **kw):
    """local_ba_cases.make_scene, then: drop_kf: that KeyFrame keeps drop_kf_edges of its edges, each with a gross error, so that
    round 1 puts all of them on level 1; drop_point: the same for all edges of that point; extra_point: one more point no edge names"""
    s = dict(lc.make_scene(seed, **kw))
    rng = np.random.default_rng(seed + 1000)
    if drop_kf is not None:
        mine = np.nonzero(s["edge_kf"] == drop_kf)[0]
        keep = np.ones(len(s["edge_kf"]), bool)
        keep[mine[drop_kf_edges:]] = False
        _keep_edges(s, keep)
        _gross(s, np.nonzero(s["edge_kf"] == drop_kf)[0], rng)
    if drop_point is not None:
        _gross(s, np.nonzero(s["edge_point"] == drop_point)[0], rng)
    if extra_point:
        s["pos_w"] = np.concatenate([s["pos_w"], s["pos_w"][-1:] + s["pos_w"].dtype.type(1.5)])
        s["depth"] = np.concatenate([s["depth"], s["depth"][-1:]])
    return s


# name -> make_scene arguments.  A scene that misses a condition of tests/test_welding_ba_cpu.py is re-seeded HERE; no bound moves.
#   mixed          2 free + 1 fixed, mono and stereo edges, 15 % gross outliers: both rounds run, round 2's graph is smaller
#   clean          no edge is flagged: round 2 is the same graph without Huber
#   kf_dropped     free KeyFrame 1 keeps four edges, all gross: all go to level 1 and round 2 does not know the KeyFrame
#   one_active_kf  the same with two free KeyFrames: round 2's reduced system is one block
#   point_dropped  every edge of point 7 is gross
#   all_flagged    every edge goes to level 1: round 2 has no edge, makes no iteration, and the final flags are round 1's
#   rejected       round 1 rejects three trials (the generator of local_ba_cases' rejected_trials): push / pop before the levels
#   depth_only     the last fixed KeyFrame faces away and sees one point at its exact pinhole image: chi2 far under the threshold
#                  at the trial state, depth negative: on level 1 by the depth alone, and flagged at the end by the final depth
#   k9             nine free KeyFrames: n = 54, more than one panel of the blocked solve; the two classifications differ
#   no_edge_point  one more point that no edge names: a vertex that returns its input bits
SCENES = {
    "mixed": dict(seed=11, free=2, fixed=1, points=40, outliers=0.15),
    "clean": dict(seed=2, free=3, fixed=2, points=40, noise=0.25),
    "mono_only": dict(seed=21, free=3, fixed=2, points=40, stereo=0.0, outliers=0.1),
    "stereo_only": dict(seed=23, free=3, fixed=2, points=40, stereo=1.0, outliers=0.1),
    "kf_dropped": dict(seed=27, free=3, fixed=2, points=40, noise=0.25, drop_kf=1),
    "point_dropped": dict(seed=27, free=3, fixed=2, points=40, noise=0.25, drop_point=7),
    "one_active_kf": dict(seed=22, free=2, fixed=2, points=40, noise=0.25, drop_kf=0),
    "all_flagged": dict(seed=26, free=1, fixed=1, points=4, degree=2, stereo=1.0, outliers=1.0),
    "rejected": dict(seed=5, free=4, fixed=2, points=60, stereo=0.0, outliers=0.4, rot_deg=5.0, trans=0.5),
    "depth_only": dict(seed=27, free=3, fixed=3, points=40, noise=0.25, behind="exact"),
    "k9": dict(seed=23, free=9, fixed=3, points=80, degree=5, outliers=0.1),
    "no_edge_point": dict(seed=25, free=2, fixed=1, points=20, outliers=0.1, extra_point=True),
}
DROPPED_KF = {"kf_dropped": 1, "one_active_kf": 0}
DROPPED_POINT = {"point_dropped": 7}

# name -> (scene, name of STOPS): the flag rises in mid-call
#   stop_between       up when round 1 returns: status 3, no levels, the one classification, round 1's estimates
#   stale_chi2         ROUND 1 ENDS ON A REJECTED TRIAL: the flag rises right after the first rejected trial (iteration 2, its first
#                      trial), so status 3 and the one classification reads the chi2 of the discarded trial state and the depth of
#                      the accepted one; classifying at the accepted state gives a different flag set (test_welding_ba_cpu.py)
#   stop_round1        before round 1's third iteration: status 3 after two iterations
#   stop_round2        before round 2's fourth iteration: status 0, round 2 with three iterations
#   stop_round2_first  before round 2's first iteration: status 0, the levels are made, round 2 makes no iteration and every edge
#                      keeps the chi2 round 1's last trial left
STOP_SCENES = {
    "stop_between": ("mixed", "between"),
    "stale_chi2": ("rejected", "round1_rejected"),
    "stop_round1": ("mixed", "round1_it2"),
    "stop_round2": ("k9", "round2_it3"),
    "stop_round2_first": ("mixed", "round2_first"),
}
ALL_SCENES = tuple(SCENES) + tuple(STOP_SCENES)

_scene_cache, _ref_cache = {}, {}


def scene(name):
    if name in STOP_SCENES:
        return scene(STOP_SCENES[name][0])
    if name not in _scene_cache:
        _scene_cache[name] = make_scene(**SCENES[name])
    return _scene_cache[name]


def reference(name, variant="forward", stop=None, chi2_at="trial"):
    """the restatement's result on a named scene (one of STOP_SCENES: with its stop), computed once per process"""
    if name in STOP_SCENES and stop is None:
        stop = STOP_SCENES[name][1]
    key = (name, variant, stop, chi2_at)
    if key not in _ref_cache:
        _ref_cache[key] = welding_ba(scene(name), variant, stop, chi2_at)
    return _ref_cache[key]


def counts(r):
    """what must be equal between any two statements of the routine"""
    return (r["status"], tuple(tuple(rd[k] for k in ROUND_KEYS) for rd in r["round"]), r["n_level1"], r["n_outliers"],
            r["active_keyframes"], r["active_points"])


def costs(r):
    return [float(rd[k]) for rd in r["round"] for k in ("chi2_initial", "chi2_final")]


def cost_distance(x, y):
    """relative; two equal costs (round 2 without an edge: 0 and 0) are at distance 0"""
    return 0.0 if x == y else abs(x - y) / max(abs(x), abs(y))


def measure():
    """D: the largest difference between any two variants over the scenes (estimate_distance); cost: the same for the four costs,
    relative; per scene also whether the variants agree on the counts and on every flag of both classifications"""
    per, D, cost = {}, 0.0, 0.0
    for name in ALL_SCENES:
        s = scene(name)
        refs = [reference(name, v) for v in VARIANTS]
        d = c = 0.0
        for a in range(len(refs)):
            for b in range(a + 1, len(refs)):
                d = max(d, *estimate_distance(s, refs[a], refs[b]))
                for x, y in zip(costs(refs[a]), costs(refs[b])):
                    c = max(c, cost_distance(x, y))
        flags = all(np.array_equal(r["level1"], refs[0]["level1"]) and np.array_equal(r["outlier"], refs[0]["outlier"]) for r in refs)
        per[name] = dict(D=d, cost=c, counts_agree=len({counts(r) for r in refs}) == 1, flags_agree=flags)
        D, cost = max(D, d), max(cost, c)
    return dict(D=D, bound=16 * D, cost=cost, scenes=per)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "welding_ba_sensitivity.json")

if __name__ == "__main__":
    if "--measure" in sys.argv:
        t0 = time.perf_counter()
        m = measure()
        with open(GOLDEN, "w") as f:
            json.dump(m, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps({k: m[k] for k in ("D", "bound", "cost")}), f"{time.perf_counter() - t0:.1f} s")
        for name, v in m["scenes"].items():
            r = reference(name)
            print(f"{name:14s} D={v['D']:.2e} cost={v['cost']:.2e} counts_agree={v['counts_agree']} flags_agree={v['flags_agree']} "
                  f"E={len(r['outlier'])} {counts(r)} chi2 {[round(x, 2) for x in costs(r)]}")
    else:
        print(__doc__)
