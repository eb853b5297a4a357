"""Device time of one msorb_pose_inertial_optimization_batch call per form and number of observations:
kernel time from the device events, median and minimum of 20 calls after 5 discarded ones, and the whole call's wall time.
Writes profiles/pose_inertial_latency.json.  Needs an MI355X."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import msorb  # noqa: E402
import pose_inertial_cases as pc  # noqa: E402


def main():
    out = {}
    for form in (0, 1):
        for n in (0, 150, 300, 1200, 2048, 2049):
            sc = pc.build(500 + n, n, form, outliers=0.1)
            args = pc.flat([sc])
            ms, wall = [], []
            for _ in range(25):
                t = time.perf_counter()
                r = msorb.pose_inertial_optimization_batch(*args, timing=True)
                wall.append((time.perf_counter() - t) * 1e3)
                ms.append(r[2])
            key = "form%d_n%d" % (form, n)
            out[key] = dict(kernel_ms_min=float(np.min(ms[5:])), kernel_ms_median=float(np.median(ms[5:])),
                            call_ms_median=float(np.median(wall[5:])), iterations=r[0][0]["iterations"].tolist())
            print(key, out[key], flush=True)
    with open(os.path.join(ROOT, "profiles", "pose_inertial_latency.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
