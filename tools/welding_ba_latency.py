#!/usr/bin/env python3
"""Latency of the welding bundle adjustment of a visual map merge on the device (msorb_welding_ba: the second
Optimizer::LocalBundleAdjustment, LoopClosing.cc:1571).

Sizes: (adjustable, fixed) KeyFrames = (5, 5), (15, 10), (30, 20) with 1500 / 2500 / 4000 points, every point seen by five
KeyFrames on average, mono and stereo edges mixed, 10 % of the edges with a gross error: both rounds run, the second over the
smaller graph.

`call` = wall time through the Python mirror (marshalling, both plan builders, the upload, the read-back of the levels and every
other read-back included), `device` = device-event time from the first launch to the last classification, `stages` = device time by
stage over both rounds (MSORB_LOCAL_BA_STAGES=1, a process-wide mode: `--stages` runs it in a process of its own and adds the split
to the file the plain run wrote).  Warm-up calls first; then the median of the block medians, spread = max - min of the block medians.
`restatement` = wall time of the float64 numpy RESTATEMENT of the routine (tests/welding_ba_cases.py, 'forward') on one host
core, the median of three runs, as tools/local_ba_latency.py has it.  The restatement is not g2o and not a host build of the
engine (its kernels have none): it is vectorised numpy with Python control flow, and the column says what the same arithmetic
costs there, nothing more; its counts and flags are compared with the device's.  g2o cannot be built where this project is developed.
    python tools/welding_ba_latency.py && python tools/welding_ba_latency.py --stages       # on the GPU box"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
os.environ["MSORB_LOCAL_BA_STAGES"] = "1" if "--stages" in sys.argv else "0"
os.environ.setdefault("OMP_NUM_THREADS", "1")          # the restatement on ONE host core

import msorb  # noqa: E402
import numpy as np  # noqa: E402
import local_ba_cases as lc  # noqa: E402
import welding_ba_cases as wc  # noqa: E402
from pose_optimization_latency import blocks, device_box, summary  # noqa: E402

ARGS = ("kf", "pos_w", "edge_kf", "edge_point", "xy", "u_right", "inv_sigma2")
STAGES = ("linearise", "schur", "solve", "trial")
SIZES = ((5, 5, 1500), (15, 10, 2500), (30, 20, 4000))


def case(adjust, fixed, points):
    return lc.make_scene(900 + adjust, free=adjust, fixed=fixed, points=points, degree=5, outliers=0.1)


def call(s):
    return msorb.welding_ba(*(s[k] for k in ARGS), timing=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--stages", action="store_true", help="the stage split only (a process of its own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "welding_ba_latency.json"))
    a = ap.parse_args()
    doc = {"what": "ms per call; median of block medians after warm-up calls, spread = max - min of the block medians",
           "call": "through the Python mirror: marshalling + both plan builders + upload + every launch and read-back",
           "device": "device events from the first launch to the last classification",
           "stages": "device events around each stage, both rounds added (MSORB_LOCAL_BA_STAGES=1, a run of its own): linearise = errors, "
                     "Jacobians and the per-vertex sums; schur = point inverses, zeroing S and the block-pair sums; solve = the blocked "
                     "L D L^T; trial = update, errors, cost",
           "restatement_numpy_one_core": "tests/welding_ba_cases.py: a numpy RESTATEMENT of the routine on one host core, median of "
                                         "three runs; NOT g2o and not a host build of the engine",
           "not_measured": "g2o (it cannot be built here); a host build of the engine (its kernels have none)",
           "box": device_box(), "sizes": []}
    for adjust, fixed, points in SIZES:
        s = case(adjust, fixed, points)
        for _ in range(a.warm):
            r = call(s)
        res = r["result"]
        x = {"adjustable_keyframes": adjust, "fixed_keyframes": fixed, "points": points, "edges": len(s["edge_kf"]),
             "status": int(res["status"]), "n_level1": int(res["n_level1"]), "n_outliers": int(res["n_outliers"]),
             "active_keyframes": int(res["active_keyframes"]), "active_points": int(res["active_points"]),
             "rounds": [{k: int(res["round"][i][k]) for k in ("iterations", "trials", "rejected_trials")} for i in range(2)]}
        if a.stages:
            per = {k: [] for k in STAGES}
            for _ in range(a.rounds):
                acc = {k: [] for k in STAGES}
                for _ in range(a.block):
                    call(s)
                    for k, v in msorb.welding_ba_stage_ms().items():
                        acc[k].append(v)
                for k in STAGES:
                    per[k].append(statistics.median(acc[k]))
            x["stages"] = {k: summary(v) for k, v in per.items()}
            print(f"({adjust}, {fixed}) P={points} E={x['edges']}: " + " ".join(f"{k} {x['stages'][k]['median_ms']:.3f}" for k in STAGES), flush=True)
        else:
            wall, dev = [], []
            for _ in range(a.rounds):
                wall += blocks(lambda: call(s), 1, a.block)
                dev.append(statistics.median(call(s)["elapsed_ms"] for _ in range(a.block)))
            x["call"], x["device"] = summary(wall), summary(dev)
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                ref = wc.welding_ba(s, "forward")
                host.append((time.perf_counter() - t0) * 1e3)
            x["restatement_numpy_one_core"] = {"median_ms": statistics.median(host), "spread_ms": max(host) - min(host), "runs": 3}
            x["flags_equal_restatement"] = bool(np.array_equal(ref["outlier"], r["outlier"]) and np.array_equal(ref["level1"], r["level1"]))
            x["counts_equal_restatement"] = [[int(res["round"][i][k]) for k in wc.ROUND_KEYS] for i in range(2)] == \
                [[ref["round"][i][k] for k in wc.ROUND_KEYS] for i in range(2)]
            print(f"({adjust}, {fixed}) P={points} E={x['edges']}: call {x['call']['median_ms']:.3f} +- {x['call']['spread_ms']:.3f} device "
                  f"{x['device']['median_ms']:.3f} +- {x['device']['spread_ms']:.3f} rounds {x['rounds']} level1 {x['n_level1']}; restatement "
                  f"{x['restatement_numpy_one_core']['median_ms']:.0f} ms, flags equal {x['flags_equal_restatement']}", flush=True)
        doc["sizes"].append(x)
    if a.stages and os.path.exists(a.out):          # the stage run adds to the file the plain run wrote
        with open(a.out) as f:
            old = json.load(f)
        for o, n in zip(old["sizes"], doc["sizes"]):
            o["stages"] = n["stages"]
        doc = old
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
