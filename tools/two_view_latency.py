#!/usr/bin/env python3
"""Latency of msorb_two_view_reconstruct beside the same statements as C++ on the host.

Sizes: 200 hypotheses of each model over N = 100 / 500 / 2000 matches (tests/two_view_cases.make_scene: the general scene, 0.5 px
noise, 20 % outliers, as many keypoints again without a match).  Neither side can stop early: the reference has no early exit.
  call_ms       one msorb.two_view_reconstruct call through the Python mirror without the per-hypothesis outputs, host clock around
                a call that ends in a stream synchronise: the median over blocks of a block's mean, after a warm-up
  device_ms     the three launches alone, between two events on the call's stream (the entry's elapsed_ms), median
  host_ms       tools/two_view_host.cc (csrc/two_view_device.h and two_view_select.h through tests/two_view_host_path.h, g++ -O2
                -ffp-contract=off) on one thread, median of its repetitions
  host2_ms      the same with FindHomography and FindFundamental on two threads, as the reference runs them (:105-110)
The tool checks that both sides return the same ok, branch, winners, chosen hypothesis and sum of inlier counts.  Nothing is claimed
against a compiled Eigen.  Writes profiles/two_view_latency.json.
    python tools/two_view_latency.py --build-only      # g++ only, no GPU needed
    python tools/two_view_latency.py                   # on the GPU box"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ms-slam_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
EXE = os.path.join(ROOT, "tools", "_two_view_host")
SRC = os.path.join(ROOT, "tools", "two_view_host.cc")


def build(force=False):
    deps = [SRC, os.path.join(ROOT, "tests", "two_view_host_path.h")] + [os.path.join(ROOT, "ms-slam_amd", "csrc", f)
                                                                          for f in ("two_view_device.h", "two_view_select.h", "new_points_device.h")]
    if not force and os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", SRC, "-o", EXE, "-lpthread"])


def host_run(tc, sc, reps, tmp):
    path = os.path.join(tmp, "scene.bin")
    tc.write_scenes(path, [sc])
    v = subprocess.check_output([EXE, path, str(reps)], timeout=900).decode().split()
    return dict(median_ms=float(v[0]), min_ms=float(v[1]), median2_ms=float(v[2]), min2_ms=float(v[3]),
                answer=[int(x) for x in v[4:10]])


def measure(msorb, tc, sc, blocks, per_block, warmup, host_reps, tmp):
    def call(**kw):
        return msorb.two_view_reconstruct(sc["keys1"], sc["keys2"], sc["matches12"], sc["sets"], sc["cam"], sigma=sc["sigma"],
                                          h_ratio=sc["h_ratio"], **kw)
    first = call()
    r = first["result"]
    host = host_run(tc, sc, host_reps, tmp)
    same = [int(r["ok"]), int(r["branch"]), int(r["winner_h"]), int(r["winner_f"]), int(r["chosen"]), int(first["counts"].sum())] == host["answer"]
    for _ in range(warmup):
        call(hypotheses=False)
    t_call, t_dev = [], []
    for _ in range(blocks):
        t0 = time.perf_counter()
        dev = [call(hypotheses=False, timing=True)[1] for _ in range(per_block)]
        t_call.append((time.perf_counter() - t0) / per_block * 1e3)
        t_dev.append(float(np.median(dev)))
    return dict(n=int((sc["matches12"] >= 0).sum()), keypoints=[len(sc["keys1"]), len(sc["keys2"])], H=len(sc["sets"]), ok=int(r["ok"]),
                branch=int(r["branch"]), inliers_of_winner=int(r["n_inliers"]), n_good=[int(x) for x in r["n_good"][:int(r["n_motion"])]],
                same_answer_on_both_sides=bool(same), call_ms=float(np.median(t_call)), call_ms_blocks=[round(x, 4) for x in t_call],
                device_ms=float(np.median(t_dev)), host_ms=host["median_ms"], host_min_ms=host["min_ms"], host2_ms=host["median2_ms"],
                host2_min_ms=host["min2_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--per-block", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_latency.json"))
    a = ap.parse_args()
    build(force=a.build_only)
    if a.build_only:
        return
    import msorb
    import two_view_cases as tc
    if msorb.lib().msorb_device_count() <= 0:
        sys.exit("no GPU: nothing measured")
    scenes = [tc.make_scene(300 + k, n, 200, noise=0.5, outliers=0.2, unmatched=(n, n)) for k, n in enumerate((100, 500, 2000))]
    with tempfile.TemporaryDirectory() as tmp:
        rows = [measure(msorb, tc, sc, a.blocks, a.per_block, a.warmup, a.host_reps, tmp) for sc in scenes]
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next(l.split(":", 1)[1].strip() for l in f if l.startswith("model name"))
    except (OSError, StopIteration):
        pass
    rec = dict(what="msorb_two_view_reconstruct (200 hypotheses per model, 20 % outliers) through the Python mirror (call_ms, host "
                    "clock), its three launches between events (device_ms) and the same statements as C++ -O2 on the host on one "
                    "thread (host_ms) and on the reference's two (host2_ms); medians; MI355X", host_cpu=cpu, blocks=a.blocks,
               calls_per_block=a.per_block, warmup_calls=a.warmup, host_repetitions=a.host_reps, results=rows)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
