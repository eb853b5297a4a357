#!/usr/bin/env python3
"""Latency of msorb_mlpnp_ransac_batch beside a plain single-thread C++ run of the same header.

Sizes: 1, 5 and 10 relocalisation candidates of H = 35 hypotheses (what SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991) leaves)
at N = 50 and 150 correspondences, and one problem of H = 300 at N = 500; 40 % outliers (tests/mlpnp_cases.make_scene;
min_inliers above every count, so that neither side stops early).  Per size:
  call_ms     one msorb.mlpnp_ransac_batch call through the Python mirror, host clock around a call that ends in a stream
              synchronise: the median over blocks of a block's mean, after a warm-up
  device_ms   the two launches alone, between two events on the call's stream (the entry's elapsed_ms), median
  host_ms     tools/mlpnp_ransac_host.cc (csrc/mlpnp_device.h and mlpnp_select.h compiled with g++ -O2 -ffp-contract=off, one
              thread) over all hypotheses, median of its repetitions; the problems of a batch one after the other
  host_us_per_hypothesis, break_even_hypotheses   host_ms over the hypotheses, and call_ms over that: the number of hypotheses
              below which a host loop that converges early is done before the call returns
The tool checks that the two sides return the same winner and the same sum of counts (the libm of the two sides may differ in the
last place: a scene where that moves a count is reported, not hidden).  Nothing is claimed against the compiled reference.
Writes profiles/mlpnp_ransac_latency.json.
    python tools/mlpnp_ransac_latency.py --build-only      # g++ only, no GPU needed
    python tools/mlpnp_ransac_latency.py                   # on the GPU box"""
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
EXE = os.path.join(ROOT, "tools", "_mlpnp_ransac_host")
SRC = os.path.join(ROOT, "tools", "mlpnp_ransac_host.cc")


def build(force=False):
    deps = [SRC] + [os.path.join(ROOT, "ms-slam_amd", "csrc", f) for f in ("mlpnp_device.h", "mlpnp_select.h", "new_points_device.h")]
    if not force and os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", f"-I{ROOT}/ms-slam_amd/csrc", SRC, "-o", EXE])


def host_run(sc, reps, tmp):
    path = os.path.join(tmp, "scene.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", len(sc["p2d"]), len(sc["sets"]), sc["min_inliers"], sc["best_inliers_in"]) + sc["cam"].tobytes() +
                sc["p2d"].tobytes() + sc["p3d"].tobytes() + sc["max_err"].tobytes() + sc["sets"].tobytes())
    v = subprocess.check_output([EXE, path, str(reps)], timeout=600).decode().split()
    return dict(median_ms=float(v[0]), min_ms=float(v[1]), winner=int(v[2]), sum_counts=int(v[5]))


def measure(msorb, mc, scenes, blocks, per_block, warmup, host_reps, tmp):
    probs = [mc.problem_of(sc) for sc in scenes]
    first = msorb.mlpnp_ransac_batch(probs)
    host = [host_run(sc, host_reps, tmp) for sc in scenes]
    same = all(int(d["result"]["winner"]) == h["winner"] and int(d["counts"].sum()) == h["sum_counts"] for d, h in zip(first, host))
    for _ in range(warmup):
        msorb.mlpnp_ransac_batch(probs)
    t_call, t_dev = [], []
    for _ in range(blocks):
        t0 = time.perf_counter()
        dev = [msorb.mlpnp_ransac_batch(probs, timing=True)[1] for _ in range(per_block)]
        t_call.append((time.perf_counter() - t0) / per_block * 1e3)
        t_dev.append(float(np.median(dev)))
    hyps = sum(len(sc["sets"]) for sc in scenes)
    host_ms, call_ms = float(sum(h["median_ms"] for h in host)), float(np.median(t_call))
    return dict(problems=len(scenes), n=len(scenes[0]["p2d"]), H=len(scenes[0]["sets"]), hypotheses=hyps,
                largest_count=[int(d["counts"].max()) for d in first], same_answer_on_both_sides=bool(same),
                call_ms=call_ms, call_ms_blocks=[round(x, 4) for x in t_call], device_ms=float(np.median(t_dev)),
                host_ms=host_ms, host_min_ms=float(sum(h["min_ms"] for h in host)), host_us_per_hypothesis=host_ms / hyps * 1e3,
                break_even_hypotheses=call_ms / (host_ms / hyps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--per-block", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlpnp_ransac_latency.json"))
    a = ap.parse_args()
    build(force=a.build_only)
    if a.build_only:
        return
    import msorb
    import mlpnp_cases as mc
    if msorb.lib().msorb_device_count() <= 0:
        sys.exit("no GPU: nothing measured")
    mk = lambda seed, n, H: mc.make_scene(seed, n, H, outlier_frac=0.4, min_inliers=n)    # noqa: E731
    sizes = [[mk(300 + 20 * k + 100 * (n == 150) + i, n, 35) for i in range(k)] for n in (50, 150) for k in (1, 5, 10)]
    sizes.append([mk(900, 500, 300)])
    with tempfile.TemporaryDirectory() as tmp:
        rows = [measure(msorb, mc, scenes, a.blocks, a.per_block, a.warmup, a.host_reps, tmp) for scenes in sizes]
    cpu = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next(l.split(":", 1)[1].strip() for l in f if l.startswith("model name"))
    except (OSError, StopIteration):
        pass
    rec = dict(what="msorb_mlpnp_ransac_batch (40 % outliers) through the Python mirror (call_ms, host clock), its two launches between "
                    "events (device_ms) and the same header over all hypotheses as single-thread C++ -O2 on the host (host_ms); medians; "
                    "MI355X", host_cpu=cpu, blocks=a.blocks, calls_per_block=a.per_block, warmup_calls=a.warmup,
               host_repetitions=a.host_reps, results=rows)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
