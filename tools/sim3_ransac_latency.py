#!/usr/bin/env python3
"""Latency of msorb_sim3_ransac_batch beside a plain single-thread C++ restatement of the same loop.

Sizes: H = 300 hypotheses over N = 100 / 500 / 2000 correspondences at 50 % outliers, and a batch of 3 problems at N = 500
(tests/sim3_cases.make_scene; min_inliers above every count, so that neither side stops early).  Per size:
  call_ms     one msorb.sim3_ransac_batch call through the Python mirror, host clock around a call that ends in a stream
              synchronise: the median over blocks of a block's mean, after a warm-up
  device_ms   the two launches alone, between two events on the call's stream (the entry's elapsed_ms), median
  host_ms     tools/sim3_ransac_host.cc (csrc/sim3_device.h and sim3_select.h compiled with g++ -O2 -ffp-contract=off, one thread)
              over all H hypotheses, median of its repetitions; for the batch the three problems one after the other
The tool checks that the two sides return the same winner and the same sum of counts.  Nothing is claimed against the compiled
reference.  Writes profiles/sim3_ransac_latency.json.
    python tools/sim3_ransac_latency.py --build-only      # g++ only, no GPU needed
    python tools/sim3_ransac_latency.py                   # on the GPU box"""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ms-slam_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
EXE = os.path.join(ROOT, "tools", "_sim3_ransac_host")
SRC = os.path.join(ROOT, "tools", "sim3_ransac_host.cc")


def build(force=False):
    deps = [SRC] + [os.path.join(ROOT, "ms-slam_amd", "csrc", f) for f in ("sim3_device.h", "sim3_select.h", "new_points_device.h")]
    if not force and os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", f"-I{ROOT}/ms-slam_amd/csrc", SRC, "-o", EXE])


def host_run(sc, reps, tmp):
    path = os.path.join(tmp, "scene.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", len(sc["X1"]), len(sc["triples"]), int(sc["fix_scale"]), sc["min_inliers"], sc["best_inliers_in"]) +
                sc["cam1"].tobytes() + sc["cam2"].tobytes() + sc["X1"].tobytes() + sc["X2"].tobytes() + sc["max_err1"].tobytes() +
                sc["max_err2"].tobytes() + sc["triples"].tobytes())
    v = subprocess.check_output([EXE, path, str(reps)], timeout=600).decode().split()
    return dict(median_ms=float(v[0]), min_ms=float(v[1]), winner=int(v[2]), sum_counts=int(v[5]))


def measure(msorb, s3, scenes, blocks, per_block, warmup, host_reps, tmp):
    probs = [s3.problem_of(sc) for sc in scenes]
    first = msorb.sim3_ransac_batch(probs)
    host = [host_run(sc, host_reps, tmp) for sc in scenes]
    same = all(int(d["result"]["winner"]) == h["winner"] and int(d["counts"].sum()) == h["sum_counts"] for d, h in zip(first, host))
    for _ in range(warmup):
        msorb.sim3_ransac_batch(probs)
    t_call, t_dev = [], []
    for _ in range(blocks):
        t0 = time.perf_counter()
        dev = [msorb.sim3_ransac_batch(probs, timing=True)[1] for _ in range(per_block)]
        t_call.append((time.perf_counter() - t0) / per_block * 1e3)
        t_dev.append(float(np.median(dev)))
    return dict(problems=len(scenes), n=[len(sc["X1"]) for sc in scenes], H=[len(sc["triples"]) for sc in scenes],
                inliers_of_winner=[int(d["result"]["n_inliers"]) for d in first], same_answer_on_both_sides=bool(same),
                call_ms=float(np.median(t_call)), call_ms_blocks=[round(x, 4) for x in t_call], device_ms=float(np.median(t_dev)),
                host_ms=float(sum(h["median_ms"] for h in host)), host_min_ms=float(sum(h["min_ms"] for h in host)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--per-block", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_ransac_latency.json"))
    a = ap.parse_args()
    build(force=a.build_only)
    if a.build_only:
        return
    import msorb
    import sim3_cases as s3
    if msorb.lib().msorb_device_count() <= 0:
        sys.exit("no GPU: nothing measured")
    mk = lambda seed, n: s3.make_scene(seed, n, 300, outlier_frac=0.5, min_inliers=n)    # noqa: E731
    sizes = [[mk(200, 100)], [mk(201, 500)], [mk(202, 2000)], [mk(203, 500), mk(204, 500), mk(205, 500)]]
    with tempfile.TemporaryDirectory() as tmp:
        rows = [measure(msorb, s3, scenes, a.blocks, a.per_block, a.warmup, a.host_reps, tmp) for scenes in sizes]
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next(l.split(":", 1)[1].strip() for l in f if l.startswith("model name"))
    except (OSError, StopIteration):
        pass
    rec = dict(what="msorb_sim3_ransac_batch (H = 300, 50 % outliers) through the Python mirror (call_ms, host clock), its two launches "
                    "between events (device_ms) and the same loop over all hypotheses as single-thread C++ -O2 on the host (host_ms); "
                    "medians; MI355X", host_cpu=cpu, blocks=a.blocks, calls_per_block=a.per_block, warmup_calls=a.warmup,
               host_repetitions=a.host_reps, results=rows)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
