#!/usr/bin/env python3
"""Latency of Optimizer::OptimizeEssentialGraph4DoF on the device (msorb_essential_graph4).

The KITTI-like trajectory of tools/essential_graph_latency.py with one loop at 50 / 200 / 500 / 1024 / 1792 free KeyFrames after one
fixed one: the chain, covisibility edges to about five earlier neighbours, one loop edge; noisy measurements, optimize(20).

`call` = wall time through the Python mirror (marshalling, the plan builder, the upload and every read-back included), `device` =
device-event time from the first launch to the last, `stages` = device time by stage (MSORB_LOCAL_BA_STAGES=1, a process-wide mode:
`--stages` runs it in a process of its own and adds the split to the file the plain run wrote).  Median of the block medians,
spread = max - min of the block medians.  `host` = the same header as single-thread g++ -O2 (tests/essential_graph4_main.cc, dense
column-by-column L D L^T), the Levenberg loop alone, on the host of the machine the device is in, at the sizes where that
finishes under a second (--host-sizes).  No g2o figure: its sparse solver cannot be built where this project is developed.
    python tools/essential_graph4_latency.py && python tools/essential_graph4_latency.py --stages       # on the GPU box"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
os.environ["MSORB_LOCAL_BA_STAGES"] = "1" if "--stages" in sys.argv else "0"

import msorb  # noqa: E402
import essential_graph4_cases as ec  # noqa: E402
from pose_optimization_latency import blocks, device_box, summary  # noqa: E402

STAGES = ("linearise", "assemble", "solve", "trial")


def case(free):
    rng = np.random.default_rng(900 + free)
    n = free + 1
    edges = [(k + 1, k) for k in range(n - 1)]
    for k in range(2, n):
        for back in sorted(set(int(b) for b in rng.integers(2, 12, 4))):
            if k - back >= 0:
                edges.append((k, k - back))
    edges.append((n - 1, 0))
    sc = ec.make_graph(900 + free, n, edges, {0}, spacing=0.5)
    sc["iterations"] = ec.ITERATIONS
    return sc


def host_ms(exe, sc, repeats):
    with tempfile.TemporaryDirectory() as d:
        ec.write_scenes(os.path.join(d, "in.bin"), [sc])
        ms = []
        for _ in range(repeats):
            p = subprocess.run([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")], capture_output=True, text=True, check=True)
            ms.append(float(re.search(r" ms ([0-9.]+)", p.stdout).group(1)))
        r = ec.read_results(os.path.join(d, "out.bin"), [sc])[0]
    return ms, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[50, 200, 500, 1024, 1792])
    ap.add_argument("--host-sizes", type=int, nargs="*", default=[50, 200, 500])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--stages", action="store_true", help="the stage split only (a process of its own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essential_graph4_latency.json"))
    a = ap.parse_args()
    doc = {"what": "ms per call; median of block medians, spread = max - min of the block medians",
           "call": "through the Python mirror: marshalling + the plan builder + upload + every launch and read-back",
           "device": "device events from the first launch to the last",
           "stages": "device events around each stage (MSORB_LOCAL_BA_STAGES=1, a run of its own): linearise = the 17 errors per edge, the "
                     "Jacobians, the edge terms and the per-vertex / per-pair sums; assemble = zeroing S and scattering the blocks; solve = the "
                     "dense L D L^T; trial = update, errors, cost.  solve_share = the solve stage over the sum of the four",
           "host": "tests/essential_graph4_main.cc, g++ -O2, one thread: the Levenberg loop alone (no file I/O), median of the repeats",
           "not_measured": "g2o (its sparse solver cannot be built here)", "ldlt_block_sizes": list(msorb.ldlt_block_sizes()),
           "box": device_box(), "loop": []}
    exe = None
    if not a.stages and a.host_sizes:
        exe = os.path.join(tempfile.mkdtemp(), "essential_graph4_main")
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", os.path.join(ROOT, "tests", "essential_graph4_main.cc"), "-o", exe], check=True)
    for free in a.sizes:
        sc = case(free)
        v = msorb.eg4_vertices(*ec.vertex_records(sc))
        fn = lambda: msorb.essential_graph4(v, sc["v0"], sc["v1"], sc["meas"], iterations=sc["iterations"], timing=True)   # noqa: E731
        big = free > 300
        rounds, block, warm = (3, 3, 1) if big else (a.rounds, a.block, 3)
        for _ in range(warm):
            r = fn()
        res = r["result"]
        x = {"free_keyframes": free, "edges": len(sc["v0"]), "n": 4 * free, "iterations": int(res["iterations"]), "trials": int(res["trials"]),
             "rejected_trials": int(res["rejected_trials"]), "stop": int(res["stop"])}
        if a.stages:
            per = {k: [] for k in STAGES}
            for _ in range(rounds):
                acc = {k: [] for k in STAGES}
                for _ in range(block):
                    fn()
                    for k, val in msorb.essential_graph4_stage_ms().items():
                        acc[k].append(val)
                for k in STAGES:
                    per[k].append(statistics.median(acc[k]))
            x["stages"] = {k: summary(val) for k, val in per.items()}
            x["solve_share"] = x["stages"]["solve"]["median_ms"] / sum(x["stages"][k]["median_ms"] for k in STAGES)
            print(f"Kf={free}: " + " ".join(f"{k} {x['stages'][k]['median_ms']:.3f}" for k in STAGES) + f" solve share {x['solve_share']:.3f}", flush=True)
        else:
            call, dev = [], []
            for _ in range(rounds):
                call += blocks(fn, 1, block)
                dev.append(statistics.median(fn()["elapsed_ms"] for _ in range(block)))
            x["call"], x["device"] = summary(call), summary(dev)
            if free in a.host_sizes:
                ms, hr = host_ms(exe, sc, 3)
                x["host"] = {"median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "repeats": len(ms),
                             "iterations": hr["iterations"], "trials": hr["trials"],
                             "pose_difference_from_device": ec.pose_difference(hr["poses"], r["poses"])}
                x["host_over_device_call"] = x["host"]["median_ms"] / x["call"]["median_ms"]
            print(f"Kf={free} E={x['edges']}: call {x['call']['median_ms']:.3f} device {x['device']['median_ms']:.3f} "
                  f"(iterations {x['iterations']}, trials {x['trials']})" + (f" host {x['host']['median_ms']:.1f}" if "host" in x else ""), flush=True)
        doc["loop"].append(x)
    if a.stages and os.path.exists(a.out):          # the stage run adds to the file the plain run wrote
        with open(a.out) as f:
            old = json.load(f)
        for o, n in zip(old["loop"], doc["loop"]):
            for k, val in n.items():
                o.setdefault(k, val)
        doc = old
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
