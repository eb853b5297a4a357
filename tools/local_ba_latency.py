#!/usr/bin/env python3
"""Latency of Optimizer::LocalBundleAdjustment on the device (msorb_local_ba) at 20 / 40 / 80 free KeyFrames with 2 000 / 5 000 /
10 000 points (a third as many fixed cameras, six observations per point, 5 % gross outliers), beside the float64 numpy
RESTATEMENT of the routine (tests/local_ba_cases.py, 'forward') on one host core.  The restatement is not g2o: it is vectorised
numpy with Python control flow, and g2o cannot be built where this project is developed; the column says what the same
arithmetic costs in that form, nothing about the reference's speed.

Per size: `call` = wall time of the call through the Python mirror (ctypes marshalling, the plan builder, the upload and every
read-back included), `device` = device-event time from the first launch to the classification, `stages` = the device time by
stage (a process-wide mode of its own, MSORB_LOCAL_BA_STAGES=1, whose event pairs add to the wall time: `--stages` runs it in a
process of its own and adds the split to the file the plain run wrote), `restatement` = wall time of the numpy routine, once.
Warm clocks: 10 calls before the first block; median of the block medians, spread = max - min of the block medians.  Writes
profiles/local_ba_latency.json.
    python tools/local_ba_latency.py && python tools/local_ba_latency.py --stages            # on the GPU box"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
os.environ.setdefault("OMP_NUM_THREADS", "1")          # the restatement on ONE host core
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("MKL_NUM_THREADS", "1")
os.environ["MSORB_LOCAL_BA_STAGES"] = "1" if "--stages" in sys.argv else "0"

import msorb  # noqa: E402
import local_ba_cases as lc  # noqa: E402
from pose_optimization_latency import blocks, device_box, summary  # noqa: E402

SIZES = ((20, 2000), (40, 5000), (80, 10000))
COUNTS = ("iterations", "trials", "rejected_trials")


def case(free, points):
    return lc.make_scene(900 + free, free=free, fixed=max(free // 3, 2), points=points, degree=6, outliers=0.05)


def run(s):
    return msorb.local_ba(s["kf"], s["pos_w"], s["edge_kf"], s["edge_point"], s["xy"], s["u_right"], s["inv_sigma2"], timing=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--stages", action="store_true", help="the stage split only (a process of its own)")
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_ba_latency.json"))
    a = ap.parse_args()
    runs = []
    for free, points in SIZES:
        s = case(free, points)
        for _ in range(10):
            r = run(s)
        res = r["result"]
        x = {"free_keyframes": free, "fixed_keyframes": int(s["kf"]["fixed"].sum()), "points": points, "edges": len(s["edge_kf"]),
             "iterations": int(res["iterations"]), "trials": int(res["trials"]), "rejected_trials": int(res["rejected_trials"]),
             "n_outliers": int(res["n_outliers"])}
        if a.stages:
            per = {k: [] for k in ("linearise", "schur", "solve", "trial")}
            for _ in range(a.rounds):
                acc = {k: [] for k in per}
                for _ in range(a.block):
                    run(s)
                    for k, v in msorb.local_ba_stage_ms().items():
                        acc[k].append(v)
                for k in per:
                    per[k].append(statistics.median(acc[k]))
            x["stages"] = {k: summary(v) for k, v in per.items()}
            print(f"Kf={free} P={points} E={x['edges']}: " + " ".join(f"{k} {v['median_ms']:.3f}" for k, v in x["stages"].items()), flush=True)
        else:
            call, dev = [], []
            for _ in range(a.rounds):
                call += blocks(lambda: run(s), 1, a.block)
                dev.append(statistics.median(run(s)["elapsed_ms"] for _ in range(a.block)))
            x["call"], x["device"] = summary(call), summary(dev)
            if not a.no_restatement:
                t0 = time.perf_counter()
                ref = lc.local_ba(s, "forward")
                x["restatement_numpy_one_core"] = {"ms": (time.perf_counter() - t0) * 1e3, "runs": 1}
                x["flags_equal_restatement"] = bool(np.array_equal(ref["outlier"], r["outlier"]))
                x["counts_equal_restatement"] = [int(res[k]) for k in COUNTS] == [ref[k] for k in COUNTS]
            print(f"Kf={free} P={points} E={x['edges']}: call {x['call']['median_ms']:.3f} ms, device {x['device']['median_ms']:.3f} ms, "
                  f"iterations {x['iterations']} trials {x['trials']}; restatement "
                  f"{x.get('restatement_numpy_one_core', {}).get('ms', float('nan')):.0f} ms", flush=True)
        runs.append(x)
    doc = {"what": "ms per Optimizer::LocalBundleAdjustment call (max_iterations 10); median of block medians, spread = max - min of the block medians",
           "call": "msorb_local_ba through the Python mirror: marshalling + the plan builder + upload + every launch and read-back",
           "device": "device events from the first launch to the classification",
           "stages": "device events around each stage (MSORB_LOCAL_BA_STAGES=1, a run of its own): linearise = errors, Jacobians and the "
                     "per-vertex sums; schur = point inverses and the block-pair sums; solve = the dense L D L^T; trial = update, errors, cost",
           "restatement_numpy_one_core": "tests/local_ba_cases.py: a numpy RESTATEMENT of the routine, NOT g2o (which cannot be built here)",
           "box": device_box(), "runs": runs}
    if a.stages and os.path.exists(a.out):          # the stage run adds to the file the plain run wrote
        with open(a.out) as f:
            doc = json.load(f)
        for old, new in zip(doc["runs"], runs):
            old["stages"] = new["stages"]
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
