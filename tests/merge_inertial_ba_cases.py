"""Optimizer::MergeInertialBA (src/Optimizer.cc:3918-4420) after its gathering loops, restated in float64 / float32 numpy for pinhole
KeyFrames without a second camera: the welding bundle adjustment of two inertial maps.  The graph: both temporal windows and the
covisible KeyFrame an inertial edge reaches have pose, velocity and both biases (kind 0, 15 unknowns); every other covisible KeyFrame
has a free pose alone, because g2o's active set leaves out the velocity and bias vertices no edge reaches (kind 3, 6 unknowns); one
KeyFrame is fixed.  EdgeInertial (Huber sqrt(16.92), the information as given), EdgeGyroRW / EdgeAccRW, EdgeMono / EdgeStereo with
mvInvLevelSigma2[octave]; setUserLambdaInit(1e3), optimize(8) with the stop flag where g2o calls terminate(); the classification
by chi2 alone (:4322-4349), read without computeError() and so at the copy the last trial wrote.

The edges' restatements, the records and the scene generator are those of tests/local_inertial_ba_cases.py and
tests/pose_inertial_cases.py, the system, the Schur complement and the update those of tests/full_inertial_ba_cases.py over the
unknown layout stated here; the graph, the loop, the classification and the scene list are stated here.  No GPU, no library and no
code shared with ms-slam_amd/csrc.

`python tests/merge_inertial_ba_cases.py --measure` writes tests/golden/merge_inertial_ba_sensitivity.json: D per quantity is the
largest difference between the first of VARIANTS (THE restatement) and any other over the scene list."""
import functools
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from inertial_opt_cases import DBL_MAX, F32, F64, ordered_sum  # noqa: E402
import full_inertial_ba_cases as fc  # noqa: E402
import local_inertial_ba_cases as lc  # noqa: E402
import pose_inertial_cases as pic  # noqa: E402

MARGIN = lc.MARGIN
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_inertial_ba_sensitivity.json")
VARIANTS = lc.VARIANTS
QUANTITIES = ("Rwb", "twb", "v", "bg", "ba", "points", "chi2", "cost")
CAPACITY = 7168                    # msorb_merge_inertial_ba_capacity(): unknowns
LAMBDA_INIT = 1e3                  # :4047
ITERATIONS = 8                     # :4317
CHI2_MONO, CHI2_STEREO = F32(5.991), F32(7.815)   # :4217, :4219


# ------------------------------------------------------------------------------------------------ the graph
def graph(sc):
    """the vertices and the active edges of one call, in the form full_inertial_ba_cases' linearise / solve_trial / apply_update read"""
    kind = sc["kf"]["kind"]
    K = len(kind)
    reached = np.zeros(K, bool)
    reached[sc["edge_kf"]] = True
    for E in sc["ie"]:
        reached[[int(E["pre"]["kf_prev"]), int(E["pre"]["kf_cur"])]] = True
    free = np.flatnonzero(((kind == 0) | (kind == 3)) & reached)                # a free KeyFrame no edge reaches is no vertex
    free_of = np.full(K, -1)
    free_of[free] = np.arange(len(free))
    Kf = len(free)
    inert = np.cumsum(kind[free] == 0) - 1
    idx = [np.concatenate([6 * i + np.arange(6), 6 * Kf + 9 * inert[i] + np.arange(9)]) if kind[k] == 0 else 6 * i + np.arange(6)
           for i, k in enumerate(free)]
    n = 6 * Kf + 9 * int((kind[free] == 0).sum())
    P = len(sc["pos"])
    included = np.zeros(P, bool)
    if len(sc["edge_kf"]):
        included[sc["edge_pt"][free_of[sc["edge_kf"]] >= 0]] = True
    keep = included[sc["edge_pt"]] if len(sc["edge_pt"]) else np.zeros(0, bool)
    new_of = np.cumsum(included) - 1
    sub = dict(sc, pos=sc["pos"][included], edge_kf=sc["edge_kf"][keep], edge_pt=new_of[sc["edge_pt"][keep]].astype(np.int64),
               xy=sc["xy"][keep], ur=sc["ur"][keep], inv=sc["inv"][keep])
    active = [free_of[int(E["pre"]["kf_prev"])] >= 0 or free_of[int(E["pre"]["kf_cur"])] >= 0 for E in sc["ie"]]
    return dict(init=0, free=free, free_of=free_of, Kf=Kf, per=9, idx=idx, nb=n, n=n, included=included, keep=keep, sub=sub, active=active,
                n_active=int(keep.sum()) + sum(active))


def validate(sc):
    """the refusals of the C entry that concern the graph -> None, "invalid" or "capacity" """
    kind = sc["kf"]["kind"]
    if ((kind < 0) | (kind > 3)).any():
        return "invalid"
    n_in, n_out = np.zeros(len(kind), int), np.zeros(len(kind), int)
    for E in sc["ie"]:
        a, c = int(E["pre"]["kf_prev"]), int(E["pre"]["kf_cur"])
        if a == c or kind[a] >= 2 or kind[c] >= 2:
            return "invalid"
        n_out[a] += 1
        n_in[c] += 1
    if (n_in > 1).any() or (n_out > 1).any():
        return "capacity"
    nxt = {int(E["pre"]["kf_prev"]): int(E["pre"]["kf_cur"]) for E in sc["ie"]}
    walked = 0
    for k in range(len(kind)):
        if n_in[k] == 0:
            while k in nxt:
                k = nxt[k]
                walked += 1
    if walked != len(sc["ie"]):
        return "capacity"
    return "capacity" if graph(sc)["n"] > CAPACITY else None


def optimize(sc, variant=VARIANTS[0], stop_trials=-1, stop_iteration=-1):
    """One call -> dict(status, iterations, trials, rejected_trials, chi2_initial, chi2_final, lambda_final, st, pts [P, 3] (all the
    caller's points), included [P], flags [E] (all the caller's edges), chi2 / thr (of the edges that count, as the classification
    reads them), decision_margin).  stop_trials / stop_iteration: the stop flag is raised once that many trials have been made /
    before that iteration (0 = it is set before optimize(), or rises before the first iteration: status 3)."""
    order = variant[0]
    G = graph(sc)
    st, pts_all = lc.initial_state(sc)
    E_all = len(sc["edge_kf"])
    out = dict(iterations=0, trials=0, rejected_trials=0, chi2_initial=0.0, chi2_final=0.0, lambda_final=0.0, n_outliers=0, flags=np.zeros(E_all, bool),
               chi2=np.zeros(0), thr=np.zeros(0), decision_margin=float("inf"), solver_failures=0)
    nothing = G["Kf"] == 0
    if nothing or stop_trials == 0 or stop_iteration == 0:
        return dict(out, status=2 if nothing else 3, st=st, pts=pts_all, included=np.zeros(len(pts_all), bool))
    pts = pts_all[G["included"]]
    n = G["n"]
    max_it = int(sc["iterations"]) if int(sc["iterations"]) > 0 else ITERATIONS
    lam, ni, n_bad, ok = 0.0, 2.0, 0, G["n_active"] > 0
    iterations = trials = rejected = failures = 0
    dmargin = float("inf")
    x = np.zeros(n)
    chi2_initial = chi2_final = 0.0
    last_chi2 = None

    def stopped():
        return (stop_trials >= 0 and trials >= stop_trials) or (stop_iteration >= 0 and iterations >= stop_iteration)
    for it in range(max_it):
        if stopped() or not ok:                                                # sparse_optimizer.cpp:376
            break
        L = fc.linearise(sc, G, st, pts, None, variant)
        current = ini = L["cost"]
        if it == 0:
            chi2_initial = current
            lam, ni, n_bad = LAMBDA_INIT, 2.0, 0
        rho, qmax = 0.0, 0
        while True:
            x, xl, solved = fc.solve_trial(G, L, lam, variant, x)
            st2, pts2, _ = fc.apply_update(sc, G, st, pts, None, x, xl, variant)
            _, _, c2 = lc.visual_errors(G["sub"], st2, pts2)
            last_chi2 = c2                                                     # what chi2() returns until the next computeError()
            temp = fc.total_cost(sc, G, c2, fc.inertial_terms(sc, G, st2, None, variant, False), None, order)
            if not solved:
                temp = DBL_MAX
                failures += 1
            scale = 0.0
            for i in range(G["Kf"]):
                for j in G["idx"][i]:
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
                st, pts = st2, pts2
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
    if iterations == 0:                                                        # the flag rose before the first iteration: handed back
        return dict(out, status=3, st=lc.initial_state(sc)[0], pts=pts_all, included=np.zeros(len(pts_all), bool))
    # ---- the classification (:4322-4349): chi2 alone, no depth test
    thr = np.where(G["sub"]["ur"] >= 0, float(CHI2_STEREO), float(CHI2_MONO))
    flags = np.zeros(E_all, bool)
    flags[G["keep"]] = last_chi2 > thr
    kind = sc["kf"]["kind"]
    st0, _ = lc.initial_state(sc)
    for k in range(len(st)):                                                   # :4398-4406: a pose-only KeyFrame's velocity and biases come back
        if kind[k] == 3:
            st[k] = dict(st[k], v=st0[k]["v"], bg=st0[k]["bg"], ba=st0[k]["ba"])
    pts_all = pts_all.copy()
    pts_all[G["included"]] = pts
    return dict(out, status=0, iterations=iterations, trials=trials, rejected_trials=rejected, chi2_initial=chi2_initial, chi2_final=chi2_final,
                lambda_final=lam, st=st, pts=pts_all, included=G["included"], flags=flags, n_outliers=int(flags.sum()), chi2=last_chi2, thr=thr,
                decision_margin=dmargin, solver_failures=failures)


# ------------------------------------------------------------------------------------------------ scenes
def build(seed, shape, n_points, iterations=3, fixed_kind=1, cut=(), idle=False, depth_negative=False, stop_trials=-1, stop_iteration=-1, **kw):
    """shape = (current window, covisible with inertial vertices, pose-only covisible, merge window): one chain of
    local_inertial_ba_cases.build's generator, [the fixed KeyFrame | the merge window | the covisible KeyFrame before the current
    window | the current window], with the link into the covisible KeyFrame left out (two maps), then the pose-only covisible
    KeyFrames beside the chain (kind 3).  fixed_kind = 2: the fixed KeyFrame has no inertial vertices and its link is absent.
    cut: further links left out, by the index of the KeyFrame they end at.  idle: one more kind 3 KeyFrame without any edge, and
    one more point with a single edge, at the fixed KeyFrame.  depth_negative: point 0 keeps one mono edge at a free KeyFrame, lies
    behind that camera and is observed exactly where it projects."""
    wc, ci, npose, wm = shape
    assert ci == 1
    n_free = wm + ci + wc
    sc = lc.build(seed, n_free, n_points, n_fixed=npose, iterations=iterations, **kw)
    kf = sc["kf"].copy()
    kf["kind"][1 + n_free:] = 3
    kf["kind"][0] = fixed_kind
    ie = sc["ie"].copy()
    ie["huber"], ie["downweight"] = 1, 0                                       # :4168-4170; no information() * 1e-2
    gone = {wm + 1} | set(cut) | ({1} if fixed_kind == 2 else set())
    links = [m for m in range(len(ie)) if int(ie[m]["pre"]["kf_cur"]) not in gone]
    ie = ie[links]
    pos, ek, ep, xy, ur, inv, octave = (sc[k].copy() for k in ("pos", "edge_kf", "edge_pt", "xy", "ur", "inv", "octave"))
    if depth_negative:
        m = np.flatnonzero((ep == 0) & (kf["kind"][ek] == 0))[:1]
        assert len(m) == 1
        k = int(ek[m[0]])
        drop = (ep == 0) & (np.arange(len(ep)) != m[0])
        ek, ep, xy, ur, inv, octave = (a[~drop] for a in (ek, ep, xy, ur, inv, octave))
        e = int(np.flatnonzero(ep == 0)[0])
        Rcw, tcw = kf[k]["Rcw"].reshape(3, 3), kf[k]["tcw"]
        Xc = np.array([0.3, 0.2, -6.0])
        pos[0] = (Rcw.T @ (Xc - tcw)).astype(F32)
        Xc = Rcw @ pos[0].astype(F64) + tcw
        xy[e] = [float(kf[k]["fx"]) * Xc[0] / Xc[2] + float(kf[k]["cx"]), float(kf[k]["fy"]) * Xc[1] / Xc[2] + float(kf[k]["cy"])]
        ur[e], inv[e], octave[e] = -1.0, 1.0, 0
    if idle:
        kf = np.concatenate([kf, kf[-1:]])                                     # a pose-only KeyFrame no edge reaches
        Rcw, tcw = kf[0]["Rcw"].reshape(3, 3), kf[0]["tcw"]
        Xc = np.array([0.5, 0.3, 10.0])
        pos = np.concatenate([pos, (Rcw.T @ (Xc - tcw)).astype(F32)[None]])
        ek, ep = np.append(ek, 0).astype(np.int32), np.append(ep, len(pos) - 1).astype(np.int32)
        uv = [float(kf[0]["fx"]) * Xc[0] / Xc[2] + float(kf[0]["cx"]) + 0.4, float(kf[0]["fy"]) * Xc[1] / Xc[2] + float(kf[0]["cy"]) - 0.3]
        xy, ur, inv, octave = np.concatenate([xy, np.asarray([uv], F32)]), np.append(ur, F32(-1)), np.append(inv, F32(1)), np.append(octave, 0).astype(np.int32)
    return dict(iterations=int(iterations), kf=kf, ie=ie, pos=pos.astype(F32), edge_kf=ek, edge_pt=ep, xy=xy.astype(F32), ur=ur.astype(F32),
                inv=inv.astype(F32), octave=octave, depth=sc["depth"], speed=sc["speed"], planted=sc["planted"], shape=shape,
                stop_trials=stop_trials, stop_iteration=stop_iteration, C15=sc["C15"][links])


# name -> (seed, shape, points, keywords).  The cost has steps of about 1e-7 of its value (the preintegration's bias correction is
# float32), so the scenes stop before Levenberg has converged to that floor (decision_margin, checked by the CPU test).
_SCENES = {
    "small": (601, (2, 1, 2, 2), 60, dict(mono_frac=0.5, start=3.0)),
    "no_cov": (602, (3, 1, 0, 3), 40, dict(start=3.0)),
    "pose_only_many": (603, (1, 1, 8, 1), 60, dict(start=3.0)),
    "fixed_pose_only": (604, (2, 1, 2, 2), 40, dict(fixed_kind=2, start=3.0)),
    "broken_link": (605, (3, 1, 2, 2), 40, dict(cut=(5,), start=3.0)),
    "idle_cov": (606, (2, 1, 2, 2), 40, dict(idle=True, start=3.0)),
    # the reference's own 8 iterations (iterations = 0) from a gross start: the fifth trial is rejected
    "outliers": (610, (2, 1, 2, 2), 80, dict(iterations=0, outliers=0.15, start=120.0, point_start=30.0)),
    "depth_negative": (608, (2, 1, 2, 2), 40, dict(depth_negative=True, start=3.0)),
    "mono_only": (609, (2, 1, 2, 2), 60, dict(mono_frac=1.0, start=3.0)),
    "stereo_only": (610, (2, 1, 2, 2), 40, dict(mono_frac=0.0, start=3.0)),
    "full": (611, (6, 1, 30, 6), 300, dict(start=3.0, obs_frac=0.3)),
    "stop_preset": (601, (2, 1, 2, 2), 60, dict(mono_frac=0.5, start=3.0, stop_trials=0)),
    # the flag after the rejected fifth trial: the flags belong to the copy that trial wrote, the estimates to the one before it
    "stop_trial": (610, (2, 1, 2, 2), 80, dict(iterations=0, outliers=0.15, start=120.0, point_start=30.0, stop_trials=5)),
    "stop_iteration": (601, (2, 1, 2, 2), 60, dict(mono_frac=0.5, start=3.0, iterations=5, stop_iteration=2)),
}
ALL = tuple(_SCENES)
# the library has no hook that raises the flag in mid-call: these run in the restatement and the host program only
DEVICE = tuple(n for n in ALL if n not in ("stop_trial", "stop_iteration"))


@functools.lru_cache(maxsize=None)
def scene(name):
    seed, shape, n_points, kw = _SCENES[name]
    return build(seed, shape, n_points, **dict(kw))


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
    return (int(r["status"]), int(r["iterations"]), int(r["trials"]), int(r["rejected_trials"]), tuple(bool(f) for f in r["flags"]),
            tuple(bool(f) for f in r["included"]), int(r["solver_failures"]))


def chi2_margin(r):
    """the smallest relative distance of a classified chi2 from its threshold"""
    return float((np.abs(r["chi2"] - r["thr"]) / r["thr"]).min()) if len(r["chi2"]) else float("inf")


def movement(sc, r):
    """how far the free vertices moved from their start, per quantity in the units of differences(): the smallest over the free
    KeyFrames that have the quantity as an unknown and over the included points"""
    if r["status"] != 0:
        return {}
    st0, pts0 = lc.initial_state(sc)
    G = graph(sc)
    kind = sc["kf"]["kind"]
    scale = dict(Rwb=1.0, twb=sc["depth"], v=max(sc["speed"], 1e-3), bg=1.0, ba=1.0)
    m = {}
    for q, u in scale.items():
        ks = [k for k in G["free"] if q in ("Rwb", "twb") or kind[k] == 0]
        m[q] = min([float(np.abs(r["st"][k][q] - st0[k][q]).max() / u) for k in ks] + [float("inf")])
    inc = np.asarray(r["included"], bool)
    m["points"] = float((np.abs(r["pts"] - pts0).max(axis=1) / sc["depth"])[inc].min()) if inc.any() else float("inf")
    return m


def from_records(rec, kf_out, pos_d, flags, included):
    st = [dict(Rwb=k["Rwb"].reshape(3, 3), twb=k["twb"], v=k["v"], bg=k["bg"], ba=k["ba"], Rcw=k["Rcw"].reshape(3, 3), tcw=k["tcw"]) for k in kf_out]
    return dict(status=int(rec["status"]), iterations=int(rec["iterations"]), trials=int(rec["trials"]), rejected_trials=int(rec["rejected_trials"]),
                n_outliers=int(rec["n_outliers"]), chi2_initial=float(rec["chi2_initial"]), chi2_final=float(rec["chi2_final"]),
                lambda_final=float(rec["lambda_final"]), st=st, pts=np.asarray(pos_d, F64).reshape(-1, 3), flags=np.asarray(flags, bool),
                included=np.asarray(included, bool), chi2=np.zeros(0), thr=np.zeros(0), solver_failures=int(rec["reserved"]))


def write_scenes(path, scenes):
    """int32 n_scenes, then per scene int32 iterations, K, NI, P, E, stop_after_trials, stop_before_iteration, 0, the records and arrays"""
    with open(path, "wb") as f:
        f.write(np.int32(len(scenes)).tobytes())
        for sc in scenes:
            f.write(np.array([sc["iterations"], len(sc["kf"]), len(sc["ie"]), len(sc["pos"]), len(sc["edge_kf"]), sc["stop_trials"],
                              sc["stop_iteration"], 0], np.int32).tobytes())
            for k, dt in (("kf", lc.KF_DTYPE), ("ie", lc.IEDGE_DTYPE), ("pos", F32), ("edge_kf", np.int32), ("edge_pt", np.int32), ("xy", F32),
                          ("ur", F32), ("inv", F32)):
                f.write(np.ascontiguousarray(sc[k], dt).tobytes())


def read_results(path, scenes):
    """per scene msorb_iba_result, msorb_iba_keyframe_out [K], the points [3 P] doubles, point_included [P], edge_outlier [E]"""
    out = []
    with open(path, "rb") as f:
        for sc in scenes:
            K, P, E = len(sc["kf"]), len(sc["pos"]), len(sc["edge_kf"])
            rec = np.frombuffer(f.read(lc.RESULT_DTYPE.itemsize), lc.RESULT_DTYPE)[0]
            ko = np.frombuffer(f.read(K * lc.KF_OUT_DTYPE.itemsize), lc.KF_OUT_DTYPE)
            pts = np.frombuffer(f.read(24 * P), F64)
            inc = np.frombuffer(f.read(P), np.uint8)
            flags = np.frombuffer(f.read(E), np.uint8)
            out.append((rec, ko, from_records(rec, ko, pts, flags, inc)))
        assert f.read() == b""
    return out


def dropin_scene(sc):
    """the scene as a map would hold it: its KeyFrames in the order a map gives them ids (the pose-only covisible KeyFrames first, then
    the chain, so that pCurrKF, the chain's last, has the largest mnId), each point's edges by ascending KeyFrame, and only the points
    a window KeyFrame observes (the others are no local points, :3992-4009) -> (scene, index of pCurrKF, of pMergeKF)"""
    wc, ci, npose, wm = sc["shape"]
    n_chain = 1 + wm + ci + wc
    K = len(sc["kf"])
    assert K == n_chain + npose
    window = np.zeros(K, bool)
    window[1:1 + wm] = window[wm + 2:n_chain] = True
    local = np.zeros(len(sc["pos"]), bool)
    local[sc["edge_pt"][window[sc["edge_kf"]]]] = True
    keep = local[sc["edge_pt"]]
    sc = dict(sc, pos=sc["pos"][local], edge_pt=(np.cumsum(local) - 1)[sc["edge_pt"][keep]].astype(np.int32),
              **{k: sc[k][keep] for k in ("edge_kf", "xy", "ur", "inv", "octave")})
    new_of = np.concatenate([npose + np.arange(n_chain), np.arange(npose)])    # old index -> new index
    kf = np.zeros(K, lc.KF_DTYPE)
    kf[new_of] = sc["kf"]
    ie = sc["ie"].copy()
    ie["pre"]["kf_prev"], ie["pre"]["kf_cur"] = new_of[ie["pre"]["kf_prev"]], new_of[ie["pre"]["kf_cur"]]
    ek = new_of[sc["edge_kf"]].astype(np.int32)
    order = np.lexsort((ek, sc["edge_pt"]))
    out = dict(sc, kf=kf, ie=ie, edge_kf=ek[order], **{k: sc[k][order] for k in ("edge_pt", "xy", "ur", "inv", "octave")})
    return out, int(new_of[n_chain - 1]), int(new_of[wm])


def write_dropin_scene(path, sc, curr, merge):
    """what tests/dropin_merge_inertial_ba_main.cc builds its stand-in map from: the records plus every edge's 15 x 15 covariance,
    the octaves and mvInvLevelSigma2"""
    assert np.array_equal(pic.LEVEL_INV_SIGMA2[sc["octave"]], sc["inv"])
    with open(path, "wb") as f:
        f.write(np.array([len(sc["kf"]), len(sc["ie"]), len(sc["pos"]), len(sc["edge_kf"]), curr, merge], np.int32).tobytes())
        for k, dt in (("kf", lc.KF_DTYPE), ("ie", lc.IEDGE_DTYPE), ("C15", F32), ("pos", F32), ("edge_kf", np.int32), ("edge_pt", np.int32), ("xy", F32),
                      ("ur", F32), ("octave", np.int32)):
            f.write(np.ascontiguousarray(sc[k], dt).tobytes())
        f.write(pic.LEVEL_INV_SIGMA2.tobytes())


DROPIN_KF = np.dtype([("n_set_pose", "<i4"), ("n_set_velocity", "<i4"), ("n_set_bias", "<i4"), ("has_corr", "<i4"), ("Rcw", "<f4", 9), ("tcw", "<f4", 3),
                      ("v", "<f4", 3), ("bias", "<f4", 6), ("corr_R", "<f8", 9), ("corr_t", "<f8", 3), ("corr_s", "<f8")])
DROPIN_PT = np.dtype([("n_set_pos", "<i4"), ("n_update", "<i4"), ("pos", "<f4", 3)])


def read_dropin_result(path, sc, gathered_only=False):
    """-> (the gathered problem as a scene dict with point_ids, dict(ret, change, n_new_bias, kf [K] records, pts [P] records, still [E]))"""
    with open(path, "rb") as f:
        assert int(np.frombuffer(f.read(4), np.int32)[0]) == 1
        its, K, NI, P, E, _, _, _ = (int(v) for v in np.frombuffer(f.read(32), np.int32))
        g = dict(iterations=its)
        g["kf"] = np.frombuffer(f.read(K * lc.KF_DTYPE.itemsize), lc.KF_DTYPE)
        g["ie"] = np.frombuffer(f.read(NI * lc.IEDGE_DTYPE.itemsize), lc.IEDGE_DTYPE)
        g["pos"] = np.frombuffer(f.read(12 * P), F32).reshape(-1, 3)
        g["edge_kf"], g["edge_pt"] = np.frombuffer(f.read(4 * E), np.int32), np.frombuffer(f.read(4 * E), np.int32)
        g["xy"] = np.frombuffer(f.read(8 * E), F32).reshape(-1, 2)
        g["ur"], g["inv"] = np.frombuffer(f.read(4 * E), F32), np.frombuffer(f.read(4 * E), F32)
        g["point_ids"] = np.frombuffer(f.read(4 * P), np.int32)
        if gathered_only:
            return g, None
        ret, change, n_new_bias = np.frombuffer(f.read(12), np.int32)
        kf = np.frombuffer(f.read(len(sc["kf"]) * DROPIN_KF.itemsize), DROPIN_KF)
        pts = np.frombuffer(f.read(len(sc["pos"]) * DROPIN_PT.itemsize), DROPIN_PT)
        still = np.frombuffer(f.read(len(sc["edge_kf"])), np.uint8).astype(bool)
        assert f.read() == b""
    return g, dict(ret=int(ret), change=int(change), n_new_bias=int(n_new_bias), kf=kf, pts=pts, still=still)


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def bounds():
    return {k: MARGIN * v for k, v in golden()["D"].items()}


def within(d, b):
    return all(d[k] <= b[k] for k in d if k in b)


def measure(names=ALL):
    """D per quantity over the scenes and the variants, and per scene its decisions, its movement, its two decision margins and its own D"""
    D = {k: 0.0 for k in QUANTITIES}
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
        per_scene[nm] = dict(decisions=[int(v) for v in decisions(base)[:4]] + [int(base["n_outliers"])], movement=movement(sc, base),
                             decision_margin=min(base["decision_margin"], 1e300), chi2_margin=min(chi2_margin(base), 1e300), D=own)
    return dict(D=D, variants_agree=agree, margin=MARGIN, variants=[list(v) for v in VARIANTS], scenes=per_scene)


if __name__ == "__main__":
    if "--measure" in sys.argv:
        m = measure()
        with open(GOLDEN, "w") as f:
            json.dump(m, f, indent=1, sort_keys=True)
        print(json.dumps(m, indent=1, sort_keys=True))
