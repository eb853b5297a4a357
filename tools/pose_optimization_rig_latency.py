#!/usr/bin/env python3
"""Latency of Optimizer::PoseOptimization of a two-camera frame on the device (msorb_pose_optimization_rig_batch: one upload, one
launch, one read-back) at N = 500 / 1200 / 2000 observations of a KannalaBrandt8 rig, half seen by the left camera and half by the
right, 15 % gross outliers, and of one fisheye-mono frame (1200 observations, one camera).  The pinhole entry
(msorb_pose_optimization_batch, tests/pose_opt_cases.py scenes of the same counts, 60 % stereo edges) runs in the same process for
comparison: the two solve different problems, the columns say what each costs, not that one is the other's baseline.

Per case: `call` = wall time of the call through the Python mirror (ctypes marshalling included, the call ends in a stream
synchronise), `kernel` = device-event time of the launch alone.  Rig and pinhole are timed in alternating blocks; median of the
block medians, spread = max - min of the block medians.  No time is promised for the rig entry, and nothing is claimed against g2o.
Writes profiles/pose_optimization_rig_latency.json.
    python tools/pose_optimization_rig_latency.py            # on the GPU box"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import msorb  # noqa: E402
import pose_opt_cases as pc  # noqa: E402
import pose_opt_rig_cases as rc  # noqa: E402
from pose_optimization_latency import blocks, device_box, summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[500, 1200, 2000])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_optimization_rig_latency.json"))
    a = ap.parse_args()
    cases = [("rig", n, dict(seed=900 + n, n=n, outliers=0.15, interleaved=True)) for n in a.sizes]
    cases.append(("fisheye_mono", 1200, dict(seed=2100, n=1200, cams=("kb8",), outliers=0.15)))
    runs = []
    for kind, n, kw in cases:
        s = rc.make_rig_scene(**kw)
        p = msorb.pose_rig_problem(s["q"], s["t"], s["cams"], s["q_rl"], s["t_rl"], n)
        rig_args = (p, s["xy"], s["camera"], s["inv_sigma2"], s["pos_w"])
        sp = pc.make_scene(700 + n, n, stereo=0.6, outliers=0.15, rot_deg=1.0, trans=0.1)
        pin_args = (msorb.pose_problem(sp["q"], sp["t"], sp["cam"], n), sp["xy"], sp["u_right"], sp["inv_sigma2"], sp["pos_w"])
        rig = lambda: msorb.pose_optimization_rig_batch(*rig_args)                       # noqa: E731
        pin = lambda: msorb.pose_optimization_batch(*pin_args)                           # noqa: E731
        for _ in range(20):
            (r,), _ = rig()
            (rp,), _ = pin()
        rig_meds, pin_meds, rig_kernel, pin_kernel = [], [], [], []
        for _ in range(a.rounds):                      # alternating blocks
            rig_meds += blocks(rig, 1, a.block)
            pin_meds += blocks(pin, 1, a.block)
            rig_kernel.append(statistics.median(msorb.pose_optimization_rig_batch(*rig_args, timing=True)[2] for _ in range(a.block)))
            pin_kernel.append(statistics.median(msorb.pose_optimization_batch(*pin_args, timing=True)[2] for _ in range(a.block)))
        runs.append({"case": kind, "n": n, "right_share": float(s["camera"].mean()), "outlier_share": 0.15, "n_bad": int(r["n_bad"]),
                     "iterations": r["iterations"].tolist(), "rejected_trials": r["rejected_trials"].tolist(),
                     "rig_entry": {"call": summary(rig_meds), "kernel": summary(rig_kernel)},
                     "pinhole_entry_same_count": {"n_bad": int(rp["n_bad"]), "iterations": rp["iterations"].tolist(),
                                                  "rejected_trials": rp["rejected_trials"].tolist(),
                                                  "call": summary(pin_meds), "kernel": summary(pin_kernel)}})
        x = runs[-1]
        print(f"{kind:13s} N={n:5d}: rig entry {x['rig_entry']['call']['median_ms']:.4f} ms (kernel {x['rig_entry']['kernel']['median_ms']:.4f}) | "
              f"pinhole entry {x['pinhole_entry_same_count']['call']['median_ms']:.4f} ms (kernel "
              f"{x['pinhole_entry_same_count']['kernel']['median_ms']:.4f}) | iterations {x['iterations']} rejected {x['rejected_trials']}", flush=True)
    doc = {"what": "wall ms per Optimizer::PoseOptimization call; median of block medians, spread = max - min of the block medians; the rig "
                   "entry and the pinhole entry alternate in one process",
           "rig_entry": "msorb_pose_optimization_rig_batch through the Python mirror: KannalaBrandt8 cameras, mono edges only",
           "pinhole_entry_same_count": "msorb_pose_optimization_batch on a pinhole scene of the same count (60 % stereo edges): another problem",
           "kernel": "device events around the launch", "box": device_box(), "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
