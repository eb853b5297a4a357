#!/usr/bin/env python3
"""Latency of Optimizer::PoseOptimization on the device (msorb_frame_pose_optimization: the keypoints resident on the frame
handle, one upload of indices and positions, one launch, one read-back) at N = 500 / 1200 / 2000 observations with 15 % gross
outliers, beside the float64 numpy RESTATEMENT of the routine (tests/pose_opt_cases.py) on one host core.  The restatement is
not g2o: it is vectorised numpy with Python control flow, and g2o cannot be built where this project is developed; the column
says what the same arithmetic costs in that form, nothing about the reference's speed.

Per size: `frame_form` = wall time of the call through the Python mirror (ctypes marshalling included, the call ends in a
stream synchronise), `kernel` = device-event time of the launch alone (flat form, same data), `restatement` = wall time of the
numpy routine.  Device and host are timed in alternating blocks in one process; median of the block medians, spread = max - min
of the block medians.  Writes profiles/pose_optimization_latency.json.
    python tools/pose_optimization_latency.py            # on the GPU box"""
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

import msorb  # noqa: E402
import pose_opt_cases as pc  # noqa: E402
from kf_database_latency import box  # noqa: E402

BOUNDS = (-400.0, 1700.0, -400.0, 800.0)     # the gross outliers leave the image


def case(n, seed, n_levels=8):
    """a frame of n / 0.6 keypoints of which n carry the observations of a scene with 15 % outliers"""
    s = pc.make_scene(seed, n, stereo=0.6, outliers=0.15, rot_deg=1.0, trans=0.1)
    rng = np.random.default_rng(seed + 1)
    n_keys = int(n / 0.6)
    slots = np.sort(rng.choice(n_keys, n, replace=False))
    scale = (1.2 ** np.arange(n_levels)).astype(np.float32)
    inv_level = (1.0 / scale.astype(np.float64) ** 2).astype(np.float32)
    kps = np.zeros(n_keys, msorb.KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, 1241, n_keys), rng.uniform(0, 376, n_keys)
    kps["octave"] = rng.integers(0, n_levels, n_keys)
    ur = np.full(n_keys, -1, np.float32)
    kps["x"][slots], kps["y"][slots], ur[slots] = s["xy"][:, 0], s["xy"][:, 1], s["u_right"]
    s["inv_sigma2"] = inv_level[kps["octave"][slots]]
    has = np.zeros(n_keys, np.uint8)
    has[slots] = 1
    pos = np.zeros((n_keys, 3), np.float32)
    pos[slots] = s["pos_w"]
    desc = rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)
    frame = msorb.Frame(kps, desc, ur, BOUNDS, scale)
    return s, frame, has, pos, inv_level


def device_box():
    info = box()
    if not info.get("gpu") or info["gpu"] == "unknown":     # rocminfo without marketing names: ask the runtime
        try:
            import torch
            info["gpu"] = torch.cuda.get_device_name(0)
            info["gpus_visible"] = torch.cuda.device_count()
        except Exception:  # noqa: BLE001
            pass
    return info


def blocks(fn, rounds, block):
    med = []
    for _ in range(rounds):
        t = []
        for _ in range(block):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        med.append(statistics.median(t))
    return med


def summary(meds):
    return {"median_ms": statistics.median(meds), "spread_ms": max(meds) - min(meds), "blocks": len(meds)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[500, 1200, 2000])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--host-block", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_optimization_latency.json"))
    a = ap.parse_args()
    runs = []
    for n in a.sizes:
        s, frame, has, pos, inv_level = case(n, 700 + n)
        p = msorb.pose_problem(s["q"], s["t"], s["cam"], n)
        dev = lambda: frame.pose_optimization(s["q"], s["t"], s["cam"], has, pos, inv_level)      # noqa: E731
        host = lambda: pc.pose_optimization(s["cam"], s["q"], s["t"], s["xy"], s["u_right"], s["inv_sigma2"], s["pos_w"])   # noqa: E731
        for _ in range(20):
            r, _ = dev()
        ref = host()
        same = bool(np.array_equal(r["q"], ref["q"]) and np.array_equal(r["t"], ref["t"]) and r["n_bad"] == ref["n_bad"])
        dev_meds, host_meds, kernel = [], [], []
        for _ in range(a.rounds):                      # alternating blocks
            dev_meds += blocks(dev, 1, a.block)
            host_meds += blocks(host, 1, a.host_block)
            kernel.append(statistics.median(msorb.pose_optimization_batch(p, s["xy"], s["u_right"], s["inv_sigma2"], s["pos_w"],
                                                                          timing=True)[2] for _ in range(a.block)))
        runs.append({"n": n, "outlier_share": 0.15, "n_bad": int(r["n_bad"]), "iterations": r["iterations"].tolist(),
                     "rejected_trials": r["rejected_trials"].tolist(), "float_pose_equals_restatement": same,
                     "frame_form": summary(dev_meds), "kernel": summary(kernel), "restatement_numpy_one_core": summary(host_meds)})
        x = runs[-1]
        print(f"N={n:5d}: frame form {x['frame_form']['median_ms']:.4f} ms (kernel {x['kernel']['median_ms']:.4f}) | numpy restatement, one core "
              f"{x['restatement_numpy_one_core']['median_ms']:.2f} ms | iterations {x['iterations']} rejected {x['rejected_trials']}", flush=True)
        frame.close()
    doc = {"what": "wall ms per Optimizer::PoseOptimization call; median of block medians, spread = max - min of the block medians; device and "
                   "host alternate in one process",
           "frame_form": "msorb_frame_pose_optimization through the Python mirror: marshalling + one upload + one launch + one read-back",
           "kernel": "device events around the launch of msorb_pose_optimization_batch on the same observations",
           "restatement_numpy_one_core": "tests/pose_opt_cases.py: a numpy RESTATEMENT of the routine, NOT g2o (which cannot be built here)",
           "box": device_box(), "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
