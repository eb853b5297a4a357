#!/usr/bin/env python3
"""Latency of Optimizer::LocalInertialBA on the device (msorb_local_inertial_ba) at 2, 10 and 25 free KeyFrames (one fixed KeyFrame
before the window, 3 / 6 / 6 fixed observers, 100 / 600 / 1000 points, 5 % gross outliers; 25 free KeyFrames run as bLarge), beside
the HOST PROGRAM: tests/local_inertial_ba_main.cc, the kernel's own text compiled by g++ -O2 and run on one core.  That is the same
arithmetic in serial form, not g2o: g2o cannot be built where this project is developed, and its speed was not measured.

Per size: `call` = wall time of the call through the Python mirror (ctypes marshalling, the plan builder, the upload and the
read-back included), `device` = device-event time of the one launch, `host_program` = the routine's time inside the host program
(its own clock around the call, median of 5 runs).  Warm clocks: 10 calls before the first block; median of the block medians,
spread = max - min of the block medians.  Writes profiles/local_inertial_ba_latency.json.
    python tools/local_inertial_ba_latency.py            # on the GPU box"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import msorb  # noqa: E402
import local_inertial_ba_cases as lc  # noqa: E402
from pose_optimization_latency import blocks, device_box, summary  # noqa: E402

SIZES = ((2, 3, 100, False), (10, 6, 600, False), (25, 6, 1000, True))


def case(free, fixed, points, large):
    return lc.build(950 + free, free, points, n_fixed=fixed, outliers=0.05, start=10.0, large=large)


def run(s):
    return msorb.local_inertial_ba(s["kf"], s["ie"], s["pos"], s["close"], s["edge_kf"], s["edge_pt"], s["xy"], s["ur"], s["inv"],
                                   large=bool(s["large"]), iterations=int(s["iterations"]), timing=True)


def host_program(tmp, scenes):
    exe = os.path.join(tmp, "local_inertial_ba_main")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-O2", os.path.join(ROOT, "tests", "local_inertial_ba_main.cc"), "-o", exe])
    lc.write_scenes(os.path.join(tmp, "in.bin"), scenes)
    per = [[] for _ in scenes]
    for _ in range(5):
        out = subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True, capture_output=True, text=True).stdout
        for i, m in enumerate(re.findall(r"in ([0-9.]+) ms", out)):
            per[i].append(float(m))
    return [statistics.median(p) for p in per], lc.read_results(os.path.join(tmp, "out.bin"), scenes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_inertial_ba_latency.json"))
    a = ap.parse_args()
    scenes = [case(*sz) for sz in SIZES]
    with tempfile.TemporaryDirectory() as tmp:
        host_ms, host = host_program(tmp, scenes)
    runs = []
    for (free, fixed, points, large), s, hms, (rec, ko, h) in zip(SIZES, scenes, host_ms, host):
        for _ in range(10):
            r = run(s)
        res = r["result"]
        call, dev = [], []
        for _ in range(a.rounds):
            call += blocks(lambda: run(s), 1, a.block)
            dev.append(statistics.median(run(s)["elapsed_ms"] for _ in range(a.block)))
        x = {"free_keyframes": free, "fixed_keyframes": fixed + 1, "points": points, "edges": len(s["edge_kf"]), "large": large,
             "iterations": int(res["iterations"]), "trials": int(res["trials"]), "rejected_trials": int(res["rejected_trials"]),
             "n_outliers": int(res["n_outliers"]), "call": summary(call), "device": summary(dev),
             "host_program_one_core": {"ms": hms, "runs": 5},
             "counts_equal_host_program": [int(res[k]) for k in ("iterations", "trials", "rejected_trials", "n_outliers")] ==
             [int(rec[k]) for k in ("iterations", "trials", "rejected_trials", "n_outliers")]}
        print(f"Kf={free} P={points} E={x['edges']}: call {x['call']['median_ms']:.3f} ms, device {x['device']['median_ms']:.3f} ms, "
              f"iterations {x['iterations']} trials {x['trials']}; host program {hms:.3f} ms", flush=True)
        runs.append(x)
    doc = {"what": "ms per Optimizer::LocalInertialBA call (iteration limit 10, 4 with bLarge; every run entry says how many iterations it took "
                   "before Levenberg's own stop: 6, 6 and 4 here); median of block medians, "
                   "spread = max - min of the block medians",
           "call": "msorb_local_inertial_ba through the Python mirror: marshalling + the plan builder + upload + the launch + read-back",
           "device": "device events around the one launch (one workgroup of 512 threads)",
           "host_program_one_core": "tests/local_inertial_ba_main.cc: the kernel's text through g++ -O2 on one core, its own clock around "
                                    "the routine.  NOT g2o, which cannot be built here and was not measured",
           "box": device_box(), "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
