#!/usr/bin/env python3
"""Latency of Optimizer::BundleAdjustment on the device (msorb_bundle_adjustment) and of its blocked dense solve.

  against_local_ba   the problems of tools/local_ba_latency.py (20 / 40 / 80 free KeyFrames) through msorb_local_ba and through
                     msorb_bundle_adjustment (robust on, 10 iterations) in the same process: with --stages the dense-solve stage
                     of each, i.e. the one-workgroup column-by-column factorisation against the blocked one
  loop_closing       129 / 256 / 512 / 1024 free KeyFrames after one fixed one, 50 points per KeyFrame with six observations each
                     inside a window of eight KeyFrames, 40 points that close the loop, robust off, 10 iterations
                     (LoopClosing.cc:2228)
  mono_init          2 KeyFrames, 100 / 300 mono points, 20 iterations, robust on (Tracking.cc:2561)

`call` = wall time through the Python mirror (marshalling, the plan builder, the upload and every read-back included), `device` =
device-event time from the first launch to the last, `stages` = device time by stage (MSORB_LOCAL_BA_STAGES=1, a process-wide
mode: `--stages` runs it in a process of its own and adds the split to the file the plain run wrote).  Median of the block medians,
spread = max - min of the block medians.  No g2o figure: it cannot be built where this project is developed.
    python tools/bundle_adjustment_latency.py && python tools/bundle_adjustment_latency.py --stages       # on the GPU box"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
os.environ["MSORB_LOCAL_BA_STAGES"] = "1" if "--stages" in sys.argv else "0"

import msorb  # noqa: E402
import bundle_adjustment_cases as bc  # noqa: E402
import local_ba_cases as lc  # noqa: E402
from local_ba_latency import case as local_case  # noqa: E402
from pose_optimization_latency import blocks, device_box, summary  # noqa: E402

ARGS = ("kf", "pos_w", "edge_kf", "edge_point", "xy", "u_right", "inv_sigma2")
STAGES = ("linearise", "schur", "solve", "trial")


def local_ba(s):
    return msorb.local_ba(*(s[k] for k in ARGS), max_iterations=10, timing=True)


def gba(s, n_iterations, robust):
    return msorb.bundle_adjustment(*(s[k] for k in ARGS), n_iterations=n_iterations, robust=robust, timing=True)


def measure(fn, stage_fn, stages, rounds, block, warm):
    for _ in range(warm):
        r = fn()
    res = r["result"]
    x = {"iterations": int(res["iterations"]), "trials": int(res["trials"]), "rejected_trials": int(res["rejected_trials"])}
    if stages:
        per = {k: [] for k in STAGES}
        for _ in range(rounds):
            acc = {k: [] for k in STAGES}
            for _ in range(block):
                fn()
                for k, v in stage_fn().items():
                    acc[k].append(v)
            for k in STAGES:
                per[k].append(statistics.median(acc[k]))
        x["stages"] = {k: summary(v) for k, v in per.items()}
        x["solve_ms_per_trial"] = x["stages"]["solve"]["median_ms"] / max(x["trials"], 1)
    else:
        call, dev = [], []
        for _ in range(rounds):
            call += blocks(fn, 1, block)
            dev.append(statistics.median(fn()["elapsed_ms"] for _ in range(block)))
        x["call"], x["device"] = summary(call), summary(dev)
    return x


def shape(s):
    fixed = int(s["kf"]["fixed"].sum())
    return {"free_keyframes": len(s["kf"]) - fixed, "fixed_keyframes": fixed, "points": len(s["pos_w"]), "edges": len(s["edge_kf"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--stages", action="store_true", help="the stage split only (a process of its own)")
    ap.add_argument("--loop-sizes", type=int, nargs="*", default=[129, 256, 512, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bundle_adjustment_latency.json"))
    a = ap.parse_args()
    doc = {"what": "ms per call; median of block medians, spread = max - min of the block medians",
           "call": "through the Python mirror: marshalling + the plan builder + upload + every launch and read-back",
           "device": "device events from the first launch to the last",
           "stages": "device events around each stage (MSORB_LOCAL_BA_STAGES=1, a run of its own): linearise = errors, Jacobians and the "
                     "per-vertex sums; schur = point inverses, zeroing S and the block-pair sums; solve = the dense L D L^T; trial = "
                     "update, errors, cost.  solve_ms_per_trial = the solve stage over the number of trials",
           "not_measured": "g2o (it cannot be built here)", "ldlt_block_sizes": list(msorb.ldlt_block_sizes()),
           "box": device_box(), "against_local_ba": [], "loop_closing": [], "mono_init": []}

    def show(tag, x):
        body = (" ".join(f"{k} {x['stages'][k]['median_ms']:.3f}" for k in STAGES) + f" solve/trial {x['solve_ms_per_trial']:.3f}" if a.stages
                else f"call {x['call']['median_ms']:.3f} device {x['device']['median_ms']:.3f}")
        print(f"{tag}: {body} (iterations {x['iterations']}, trials {x['trials']})", flush=True)

    for free, points in ((20, 2000), (40, 5000), (80, 10000)):
        s = local_case(free, points)
        x = shape(s)
        x["local_ba"] = measure(lambda: local_ba(s), msorb.local_ba_stage_ms, a.stages, a.rounds, a.block, 10)
        x["bundle_adjustment"] = measure(lambda: gba(s, 10, True), msorb.bundle_adjustment_stage_ms, a.stages, a.rounds, a.block, 10)
        if a.stages:
            lo, bl = x["local_ba"]["stages"]["solve"], x["bundle_adjustment"]["stages"]["solve"]
            x["solve_stage_local_over_blocked"] = (x["local_ba"]["solve_ms_per_trial"] / x["bundle_adjustment"]["solve_ms_per_trial"])
            x["solve_stage_spread_ms"] = max(lo["spread_ms"], bl["spread_ms"])
        show(f"Kf={free} local_ba", x["local_ba"])
        show(f"Kf={free} bundle_adjustment", x["bundle_adjustment"])
        doc["against_local_ba"].append(x)
    for free in a.loop_sizes:
        s = bc.make_windowed_scene(700 + free, free=free, points=50 * free, degree=6, window=8, loop_points=40, outliers=0.05)
        x = shape(s)
        big = free > 200
        x.update(measure(lambda: gba(s, 10, False), msorb.bundle_adjustment_stage_ms, a.stages, 3 if big else a.rounds, 3 if big else a.block,
                         2 if big else 10))
        show(f"loop Kf={free} P={x['points']} E={x['edges']}", x)
        doc["loop_closing"].append(x)
    for points in (100, 300):
        s = lc.make_scene(800 + points, free=2, fixed=0, init_fixed=1, points=points, stereo=0.0, degree=2)
        x = shape(s)
        x.update(measure(lambda: gba(s, 20, True), msorb.bundle_adjustment_stage_ms, a.stages, a.rounds, a.block, 10))
        show(f"mono init P={points}", x)
        doc["mono_init"].append(x)
    if a.stages and os.path.exists(a.out):          # the stage run adds to the file the plain run wrote
        with open(a.out) as f:
            old = json.load(f)
        for part in ("against_local_ba", "loop_closing", "mono_init"):
            for o, n in zip(old[part], doc[part]):
                for k, v in n.items():
                    if isinstance(v, dict) and isinstance(o.get(k), dict):
                        o[k].update(v)
                    else:
                        o.setdefault(k, v)
        doc = old
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
