#!/usr/bin/env python3
"""Latency of Optimizer::MergeInertialBA on the device (msorb_merge_inertial_ba) at (window, covisible) sizes (4, 5), (12, 15) and
(12, 31) with about 1500 points: `window` KeyFrames of both temporal windows together (15 unknowns each), `covisible` KeyFrames of
which one has inertial vertices and the others a free pose alone (6 unknowns), one fixed KeyFrame, the reference's 8 iterations,
5 % gross outliers.  (12, 31) is the reference's largest graph.

Per size: `call` = wall time through the Python mirror (marshalling, the plan builder, the upload, every launch and read-back),
`device` = device-event time between the upload and the final read-back, `stages` = the per-stage split of one call with
MSORB_MERGE_INERTIAL_BA_STAGES=1 (linearise, assemble, Schur, solve, trial), `host_program` = tests/merge_inertial_ba_main.cc, the
kernels' own text through g++ -O2 on one core with the column-by-column solve (its own clock around the routine, median of 3 runs).
NOT g2o, which cannot be built where this project is developed.  Median of block medians.  Writes
profiles/merge_inertial_ba_latency.json.
    MSORB_MERGE_INERTIAL_BA_STAGES=1 python tools/merge_inertial_ba_latency.py [--cache DIR]     # on the GPU box"""
import argparse
import json
import os
import pickle
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import merge_inertial_ba_cases as mc  # noqa: E402

SIZES = ((4, 5), (12, 15), (12, 31))
POINTS = 1500


def case(window, covisible):
    return mc.build(980 + window + covisible, (window // 2, 1, covisible - 1, window // 2), POINTS, iterations=0, outliers=0.05, start=10.0, obs_frac=0.3)


def scenes(cache):
    out = []
    for sz in SIZES:
        path = cache and os.path.join(cache, "miba_latency_%d_%d.pkl" % sz)
        if path and os.path.exists(path):
            with open(path, "rb") as f:
                out.append(pickle.load(f))
            continue
        s = {k: v for k, v in case(*sz).items() if k not in ("C15", "octave", "planted")}
        if path:
            os.makedirs(cache, exist_ok=True)
            with open(path, "wb") as f:
                pickle.dump(s, f)
        out.append(s)
    return out


def host_program(sc, runs=3):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "merge_inertial_ba_main")
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-O2", os.path.join(ROOT, "tests", "merge_inertial_ba_main.cc"), "-o", exe])
        mc.write_scenes(os.path.join(tmp, "in.bin"), sc)
        per = [[] for _ in sc]
        for _ in range(runs):
            out = subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True, capture_output=True, text=True).stdout
            for i, m in enumerate(re.findall(r"in ([0-9.]+) ms", out)):
                per[i].append(float(m))
        return [statistics.median(p) for p in per], mc.read_results(os.path.join(tmp, "out.bin"), sc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--cache", default=None, help="a directory the generated scenes are kept in")
    ap.add_argument("--only-cache", action="store_true", help="generate the scenes into --cache and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_inertial_ba_latency.json"))
    a = ap.parse_args()
    sc = scenes(a.cache)
    if a.only_cache:
        return 0
    import msorb
    from pose_optimization_latency import blocks, device_box, summary

    def run(s):
        return msorb.merge_inertial_ba(s["kf"], s["ie"], s["pos"], s["edge_kf"], s["edge_pt"], s["xy"], s["ur"], s["inv"], iterations=int(s["iterations"]),
                                       timing=True)
    host_ms, host = host_program(sc)
    runs = []
    for (window, covisible), s, hms, (rec, ko, h) in zip(SIZES, sc, host_ms, host):
        G = mc.graph(s)
        for _ in range(5):
            r = run(s)
        res = r["result"]
        call, dev = [], []
        for _ in range(a.rounds):
            call += blocks(lambda: run(s), 1, a.block)
            dev.append(statistics.median(run(s)["elapsed_ms"] for _ in range(a.block)))
        counts = ("iterations", "trials", "rejected_trials", "n_outliers")
        x = {"window": window, "covisible": covisible, "free_keyframes": int(G["Kf"]), "unknowns": int(G["n"]), "points": len(s["pos"]),
             "edges": len(s["edge_kf"]), "iterations": int(res["iterations"]), "trials": int(res["trials"]), "rejected_trials": int(res["rejected_trials"]),
             "flagged": int(res["n_outliers"]), "failed_factorisations": int(res["reserved"]), "call": summary(call), "device": summary(dev),
             "host_program_one_core": {"ms": hms, "runs": 3},
             "counts_equal_host_program": [int(res[k]) for k in counts] == [int(rec[k]) for k in counts]}
        try:
            x["stages_ms"] = msorb.merge_inertial_ba_stage_ms()
        except msorb.MsorbError:
            x["stages_ms"] = None
        print(f"window={window} covisible={covisible} n={x['unknowns']} P={x['points']} E={x['edges']}: call {x['call']['median_ms']:.2f} ms, device "
              f"{x['device']['median_ms']:.2f} ms, iterations {x['iterations']} trials {x['trials']} flagged {x['flagged']}; stages {x['stages_ms']}; "
              f"host program {hms:.2f} ms, counts equal {x['counts_equal_host_program']}", flush=True)
        runs.append(x)
    doc = {"what": "ms per Optimizer::MergeInertialBA call; every run says how many iterations and trials it made; median of block medians, "
                   "spread = max - min of the block medians",
           "call": "msorb_merge_inertial_ba through the Python mirror: marshalling + the plan builder + upload + every launch and read-back",
           "device": "device events from after the upload to before the final read-back (the host's per-trial read-backs included)",
           "stages_ms": "one call's device time per stage, MSORB_MERGE_INERTIAL_BA_STAGES=1",
           "host_program_one_core": "tests/merge_inertial_ba_main.cc: the kernels' text through g++ -O2 on one core, column-by-column solve, its own "
                                    "clock around the routine.  NOT g2o, which cannot be built here and was not measured",
           "box": device_box(), "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
