#!/usr/bin/env python3
"""Latency of Optimizer::FullInertialBA on the device (msorb_full_inertial_ba) at the shapes of its call sites: init = 1 at 10 / 20 /
40 KeyFrames with 100 iterations asked (LocalMapping::InitializeIMU) and init = 0 at 25 / 100 / 200 / 477 KeyFrames with 7 iterations
(the global BA after a loop closure; 477 is the capacity), 5 % gross outliers, no fixed KeyFrame except in the 25-KeyFrame case: that
one is the window tools/local_inertial_ba_latency.py measures (25 free KeyFrames, 7 fixed, 1000 points), so msorb_local_inertial_ba's one-workgroup
time from profiles/local_inertial_ba_latency.json stands beside it, per iteration.

Per size: `call` = wall time through the Python mirror (marshalling, the plan builder, the upload, every launch and read-back),
`device` = device-event time between the upload and the final read-back, `stages` = the per-stage split of one call with
MSORB_FULL_INERTIAL_BA_STAGES=1 (linearise, assemble, Schur, solve, trial), `host_program` = tests/full_inertial_ba_main.cc, the
kernels' own text through g++ -O2 on one core with the column-by-column solve (its own clock around the routine; median of 3 runs up
to 400 unknowns, one run above, and only up to --host-max unknowns: the serial solve is cubic).  NOT g2o, which cannot be built where this project is developed.  Median of block
medians.  Writes profiles/full_inertial_ba_latency.json.
    MSORB_FULL_INERTIAL_BA_STAGES=1 python tools/full_inertial_ba_latency.py [--cache DIR]     # on the GPU box"""
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

import numpy as np  # noqa: E402
import full_inertial_ba_cases as fc  # noqa: E402
import local_inertial_ba_cases as lc  # noqa: E402

SIZES = ((1, 10, 400), (1, 20, 800), (1, 40, 1600), (0, 25, 1000), (0, 100, 2000), (0, 200, 2400), (0, 477, 3800))


def case(init, kfs, points):
    if (init, kfs) == (0, 25):                                                 # local_inertial_ba_latency.py's largest window
        s = lc.build(975, 25, 1000, n_fixed=6, outliers=0.05, start=10.0, large=True)
        ie = s["ie"].copy()
        ie["huber"], ie["downweight"] = 1, 0
        return dict(s, init=0, iterations=7, ie=ie, prior_g=np.float32(0), prior_a=np.float32(0), bg0=np.zeros(3), ba0=np.zeros(3),
                    stop_trials=-1, stop_iteration=-1)
    return fc.build(960 + kfs, kfs, points, init=init, iterations=100 if init else 7, outliers=0.05, start=10.0, priors=fc.PRIORS[1], bias0=1e-3)


def scenes(cache):
    out = []
    for sz in SIZES:
        path = cache and os.path.join(cache, "fiba_latency_%d_%d.pkl" % sz[:2])
        if path and os.path.exists(path):
            with open(path, "rb") as f:
                out.append(pickle.load(f))
            continue
        s = case(*sz)
        s = {k: v for k, v in s.items() if k not in ("truth", "true_points", "C15", "octave")}
        if path:
            os.makedirs(cache, exist_ok=True)
            with open(path, "wb") as f:
                pickle.dump(s, f)
        out.append(s)
    return out


def host_program(sc, runs=3):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "full_inertial_ba_main")
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-O2", os.path.join(ROOT, "tests", "full_inertial_ba_main.cc"), "-o", exe])
        fc.write_scenes(os.path.join(tmp, "in.bin"), sc)
        per = [[] for _ in sc]
        for _ in range(runs):
            out = subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True, capture_output=True, text=True).stdout
            for i, m in enumerate(re.findall(r"in ([0-9.]+) ms", out)):
                per[i].append(float(m))
        return [statistics.median(p) for p in per], fc.read_results(os.path.join(tmp, "out.bin"), sc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--cache", default=None, help="a directory the generated scenes are kept in")
    ap.add_argument("--host-max", type=int, default=1500, help="the host program runs the scenes of at most this many unknowns")
    ap.add_argument("--only-cache", action="store_true", help="generate the scenes into --cache and stop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "full_inertial_ba_latency.json"))
    a = ap.parse_args()
    sc = scenes(a.cache)
    if a.only_cache:
        return 0
    import msorb
    from pose_optimization_latency import blocks, device_box, summary

    def run(s):
        return msorb.full_inertial_ba(s["kf"], s["ie"], s["pos"], s["edge_kf"], s["edge_pt"], s["xy"], s["ur"], s["inv"], init=bool(s["init"]),
                                      iterations=int(s["iterations"]), prior_g=s["prior_g"], prior_a=s["prior_a"], bg0=s["bg0"], ba0=s["ba0"], timing=True)
    host_of = {}
    for lo, hi, runs in ((0, 400, 3), (400, a.host_max, 1)):
        pick = [i for i, s in enumerate(sc) if lo < fc.graph(s)["n"] <= hi]
        if pick:
            host_ms, host = host_program([sc[i] for i in pick], runs)
            host_of.update({i: (ms, h, runs) for i, ms, h in zip(pick, host_ms, host)})
    local = None
    try:
        with open(os.path.join(ROOT, "profiles", "local_inertial_ba_latency.json")) as f:
            local = [r for r in json.load(f)["runs"] if r["free_keyframes"] == 25][0]
    except (OSError, IndexError, KeyError):
        pass
    runs = []
    for i, ((init, kfs, points), s) in enumerate(zip(SIZES, sc)):
        n = fc.graph(s)["n"]
        reps = 1 if n > 3000 else a.block
        for _ in range(2 if n > 3000 else 5):
            r = run(s)
        res = r["result"]
        call, dev = [], []
        for _ in range(a.rounds):
            call += blocks(lambda: run(s), 1, reps)
            dev.append(statistics.median(run(s)["elapsed_ms"] for _ in range(reps)))
        x = {"init": init, "keyframes": len(s["kf"]), "free_keyframes": int((s["kf"]["kind"] == 0).sum()), "unknowns": n, "points": len(s["pos"]),
             "edges": len(s["edge_kf"]), "iterations_asked": int(s["iterations"]), "iterations": int(res["iterations"]), "trials": int(res["trials"]),
             "rejected_trials": int(res["rejected_trials"]), "failed_factorisations": int(res["reserved"]), "call": summary(call), "device": summary(dev)}
        try:
            x["stages_ms"] = msorb.full_inertial_ba_stage_ms()
        except msorb.MsorbError:
            x["stages_ms"] = None
        if i in host_of:
            ms, (rec, ko, h), host_runs = host_of[i]
            x["host_program_one_core"] = {"ms": ms, "runs": host_runs}
            x["counts_equal_host_program"] = [int(res[k]) for k in ("iterations", "trials", "rejected_trials")] == [int(rec[k]) for k in ("iterations", "trials", "rejected_trials")]
        if local is not None and (init, kfs) == (0, 25):
            x["local_inertial_ba_one_workgroup"] = {"device_ms": local["device"]["median_ms"], "iterations": local["iterations"], "trials": local["trials"]}
        print(f"init={init} K={kfs} n={n} P={x['points']} E={x['edges']}: call {x['call']['median_ms']:.2f} ms, device {x['device']['median_ms']:.2f} ms, "
              f"iterations {x['iterations']} trials {x['trials']}; stages {x['stages_ms']}; host program {x.get('host_program_one_core')}", flush=True)
        runs.append(x)
    doc = {"what": "ms per Optimizer::FullInertialBA call; every run says how many iterations and trials it made before Levenberg's own stop; "
                   "median of block medians, spread = max - min of the block medians",
           "call": "msorb_full_inertial_ba through the Python mirror: marshalling + the plan builder + upload + every launch and read-back",
           "device": "device events from after the upload to before the final read-back (the host's per-trial read-backs included)",
           "stages_ms": "one call's device time per stage, MSORB_FULL_INERTIAL_BA_STAGES=1",
           "host_program_one_core": "tests/full_inertial_ba_main.cc: the kernels' text through g++ -O2 on one core, column-by-column solve, its own "
                                    "clock around the routine.  NOT g2o, which cannot be built here and was not measured",
           "box": device_box(), "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
