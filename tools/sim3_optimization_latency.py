#!/usr/bin/env python3
"""Latency of Optimizer::OptimizeSim3 on the device (msorb_sim3_optimization_batch: one upload, one launch, one read-back) at
N = 50 / 200 / 1000 pairs with 20 % gross outliers and for a batch of three problems of N = 200, beside the SAME routine as
single-thread C++: tests/sim3_opt_main.cc over the header the kernel compiles (csrc/sim3_opt_device.h), built with
g++ -O2 -ffp-contract=off and run on this machine's host.  Nothing is claimed against g2o, which cannot be built where this
project is developed.

Per size: `call` = wall time of the call through the Python mirror (ctypes marshalling included, the call ends in a stream
synchronise), `kernel` = device-event time of the launch alone, `host_cpp_one_thread` = the stand-alone program's own median over
its repetitions (steady_clock around the routine, file I/O outside).  Device figures: median of the block medians after a
warm-up, spread = max - min of the block medians.  Writes profiles/sim3_optimization_latency.json.
    python tools/sim3_optimization_latency.py            # on the GPU box"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import msorb  # noqa: E402
import sim3_opt_cases as sc  # noqa: E402
from pose_optimization_latency import blocks, device_box, summary  # noqa: E402

ARRAYS = ("P1c", "P2c", "obs1", "obs2", "w1", "w2")
HOST_EXE = os.path.join(ROOT, "tools", "_sim3_opt_main")


def build_host():
    src = os.path.join(ROOT, "tests", "sim3_opt_main.cc")
    if not os.path.exists(HOST_EXE) or os.path.getmtime(HOST_EXE) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", HOST_EXE])


def host_ms(scenes, repeat):
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        sc.write_problems(fin, scenes)
        out = subprocess.run([HOST_EXE, fin, fout, str(repeat)], capture_output=True, text=True, check=True).stdout
        res = sc.read_results(fout, scenes)
    return [float(line.split()[-1]) for line in out.splitlines() if line.startswith("problem")], res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[50, 200, 1000])
    ap.add_argument("--batch", type=int, nargs=2, default=[3, 200], help="problems, pairs each")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--host-repeat", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_optimization_latency.json"))
    a = ap.parse_args()
    build_host()
    cases = [[sc.make_scene(900 + n, n, outliers=0.2)] for n in a.sizes]
    cases.append([sc.make_scene(950 + k, a.batch[1], outliers=0.2) for k in range(a.batch[0])])
    runs = []
    for ss in cases:
        probs = np.concatenate([msorb.sim3_opt_problem(s["q"], s["t"], s["s"], s["cam1"], s["cam2"], s["th2"], s["fix_scale"], s["min_pairs"],
                                                       len(s["w1"])) for s in ss])
        cat = [np.concatenate([np.asarray(s[k], np.float32).reshape(-1) for s in ss]) for k in ARRAYS]
        dev = lambda: msorb.sim3_optimization_batch(probs, *cat, chi2=False)                 # noqa: E731
        for _ in range(20):
            res, bad, _ = dev()
        h_ms, h_res = host_ms(ss, a.host_repeat)
        same_flags = bool(np.array_equal(bad, np.concatenate([r["bad"] for r in h_res])))
        dev_meds, kernel = [], []
        for _ in range(a.rounds):
            dev_meds += blocks(dev, 1, a.block)
            kernel.append(statistics.median(msorb.sim3_optimization_batch(probs, *cat, chi2=False, timing=True)[3] for _ in range(a.block)))
        runs.append({"problems": len(ss), "n": len(ss[0]["w1"]), "outlier_share": 0.2, "n_bad": res["n_bad"].tolist(), "n_in": res["n_in"].tolist(),
                     "iterations": res["iterations"].tolist(), "rejected_trials": res["rejected_trials"].tolist(),
                     "flags_equal_host_cpp": same_flags, "call": summary(dev_meds), "kernel": summary(kernel),
                     "host_cpp_one_thread": {"median_ms_per_problem": h_ms, "sum_ms": sum(h_ms), "repeat": a.host_repeat}})
        x = runs[-1]
        print(f"{x['problems']} x N={x['n']:5d}: call {x['call']['median_ms']:.4f} ms (kernel {x['kernel']['median_ms']:.4f}) | host C++, one thread "
              f"{x['host_cpp_one_thread']['sum_ms']:.4f} ms | iterations {x['iterations']} rejected {x['rejected_trials']}", flush=True)
    doc = {"what": "wall ms per Optimizer::OptimizeSim3 call (after the gathering loops); device: median of block medians after a warm-up, "
                   "spread = max - min of the block medians",
           "call": "msorb_sim3_optimization_batch through the Python mirror: marshalling + one upload + one launch + one read-back",
           "kernel": "device events around the launch, same data",
           "host_cpp_one_thread": "tests/sim3_opt_main.cc over csrc/sim3_opt_device.h, g++ -O2 -ffp-contract=off, steady_clock around the routine, "
                                  "median of `repeat` runs per problem; a batch is the sum of its problems.  NOT g2o (which cannot be built here)",
           "box": device_box(), "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
