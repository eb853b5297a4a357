#!/usr/bin/env python3
"""Latency of Optimizer::InertialOptimization on the device (msorb_inertial_optimization).

The first overload's problem (IMU initialisation: gravity direction, scale, biases, every velocity; mono, priors (1, 1e5),
optimize(200)) at K = 10, 50, 200, 1000 KeyFrames and the third's (ScaleRefinement: Gauss-Newton, 10 iterations, Huber) at
K = 200, 1000, on the scenes of tests/inertial_opt_cases.py's generator.

`call` = wall time through the Python mirror (marshalling, the plan, the upload, the launch and the read-back), `device` =
device-event time around the one launch.  Median of the block medians, spread = max - min of the block medians.  `host` = the same
header as single-thread g++ -O2 (tests/inertial_opt_main.cc), the optimisation alone, on the host of the machine the device is
in.  No g2o figure: it cannot be built where this project is developed.  A size where the device loses is written down as such.
    python tools/inertial_optimization_latency.py       # on the GPU box"""
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
import inertial_opt_cases as ic  # noqa: E402
from pose_optimization_latency import blocks, device_box, summary  # noqa: E402

CASES = (("first", 10), ("first", 50), ("first", 200), ("first", 1000), ("third", 200), ("third", 1000))


def host_ms(exe, sc, repeats):
    with tempfile.TemporaryDirectory() as d:
        ic.write_scenes(os.path.join(d, "in.bin"), [sc])
        ms = []
        for _ in range(repeats):
            p = subprocess.run([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")], capture_output=True, text=True, check=True)
            ms.append(float(re.search(r" ms ([0-9.]+)", p.stdout).group(1)))
        r = ic.read_results(os.path.join(d, "out.bin"), [sc])[0]
    return ms, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inertial_optimization_latency.json"))
    a = ap.parse_args()
    doc = {"what": "ms per call; median of block medians, spread = max - min of the block medians",
           "call": "through the Python mirror: marshalling + the plan + upload + the one launch + read-back",
           "device": "device events around the one launch (one workgroup of 256 threads)",
           "host": "tests/inertial_opt_main.cc, g++ -O2, one thread: the optimisation alone (no file I/O), median of the repeats",
           "not_measured": "g2o (it cannot be built here)", "box": device_box(), "cases": []}
    exe = os.path.join(tempfile.mkdtemp(), "inertial_opt_main")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", os.path.join(ROOT, "tests", "inertial_opt_main.cc"), "-o", exe], check=True)
    for overload, K in CASES:
        sc = ic.make_scene(seed=700 + K, K=K, overload=overload, priors=(1.0, 1e5))
        fn = lambda: msorb.inertial_optimization(sc["problem"], sc["kfs"], sc["edges"], timing=True)   # noqa: E731
        for _ in range(2):
            r = fn()
        res = r["result"]
        x = {"overload": overload, "keyframes": K, "edges": len(sc["edges"]), "iterations": int(res["iterations"]),
             "rejected_trials": int(res["rejected_trials"]), "status": int(res["status"])}
        call, dev = [], []
        for _ in range(a.rounds):
            call += blocks(fn, 1, a.block)
            dev.append(statistics.median(fn()["elapsed_ms"] for _ in range(a.block)))
        x["call"], x["device"] = summary(call), summary(dev)
        x["device_ms_per_solve"] = x["device"]["median_ms"] / max(1, x["iterations"] + x["rejected_trials"])
        ms, hr = host_ms(exe, sc, 3)
        x["host"] = {"median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "repeats": len(ms), "iterations": hr["iterations"],
                     "rejected_trials": hr["rejected_trials"]}
        x["host_over_device_call"] = x["host"]["median_ms"] / x["call"]["median_ms"]
        x["device_wins"] = bool(x["host_over_device_call"] > 1.0)
        print(f"{overload} K={K}: call {x['call']['median_ms']:.3f} device {x['device']['median_ms']:.3f} host {x['host']['median_ms']:.3f} "
              f"(iterations {x['iterations']}, rejected {x['rejected_trials']}; host {x['host']['iterations']}, {x['host']['rejected_trials']})",
              flush=True)
        doc["cases"].append(x)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(a.out, ROOT))


if __name__ == "__main__":
    main()
