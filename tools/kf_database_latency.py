#!/usr/bin/env python3
"""Latency of the place-recognition query on the device-resident BoW database (msorb_kf_database_query through the C ABI,
DetectRelocalizationCandidates through ms-slam_amd/host/KeyFrameDatabase_device.h) beside the same query by an inverted-file
restatement of the reference's algorithm on one host core (tools/kf_database_host_ref.h): 300 / 3 000 / 30 000 entries of about
300 words, queries of about 300 and of 2 000 words.  The three are timed in one process per size, in alternating blocks
(tools/kf_database_latency.cc); this script builds that program, runs it once per size in a fresh child process and writes
profiles/kf_database_latency.json.
    python tools/kf_database_latency.py --build-only      # g++ only, no GPU needed
    python tools/kf_database_latency.py                   # on the GPU box"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "_kf_database_latency")
SRC = [os.path.join(ROOT, "tools", f) for f in ("kf_database_latency.cc", "kf_database_host_ref.h")]


def build(force=False):
    deps = SRC + [os.path.join(ROOT, "ms-slam_amd", "host", "KeyFrameDatabase_device.h"), os.path.join(ROOT, "include", "msorb.h")]
    if not force and os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O2", f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include", f"-I{ROOT}/tools", SRC[0],
                           f"-L{ROOT}/ms-slam_amd", "-lmsorb", f"-Wl,-rpath,{ROOT}/ms-slam_amd", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                           "-o", EXE])


def box():
    info = {"gpu": "unknown", "cpu": "unknown"}
    try:
        out = subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True, timeout=60).stdout
        names = [l.split(":", 1)[1].strip() for l in out.splitlines() if "Marketing Name" in l]
        gpus = [n for n in names if "Instinct" in n or "MI3" in n]
        info["gpu"] = gpus[0] if gpus else (names[-1] if names else "unknown")
        info["gpus_visible"] = len(gpus)
    except (OSError, subprocess.SubprocessError):
        pass
    try:
        with open("/proc/cpuinfo") as f:
            info["cpu"] = next(l.split(":", 1)[1].strip() for l in f if l.startswith("model name"))
    except (OSError, StopIteration):
        pass
    return info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--entries", type=int, nargs="*", default=[300, 3000, 30000])
    ap.add_argument("--query-spans", type=int, nargs="*", default=[300, 2000])
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kf_database_latency.json"))
    a = ap.parse_args()
    build(force=a.build_only)
    if a.build_only:
        return
    runs = []
    for n in a.entries:
        for span in a.query_spans:
            line = subprocess.check_output([EXE, str(n), str(span), str(a.rounds), str(a.block)], timeout=900).decode().strip().splitlines()[-1]
            runs.append(json.loads(line))
            r = runs[-1]
            print(f"{n:6d} entries, query {r['words_per_query']:7.1f} words: abi {r['abi']['median_ms']:.4f} (kernel {r['abi_kernel_ms_median']:.4f})"
                  f" | host template {r['host_template']['median_ms']:.4f} | one host core {r['host_core']['median_ms']:.4f} ms", flush=True)
    doc = {"what": "wall ms per place-recognition query; median of block medians, spread = max - min of the block medians; "
                   "abi / host_template / host_core alternate in one process (tools/kf_database_latency.cc)",
           "split": "one kernel launch scores every sharing entry; the ordering by (first common word, add sequence), the maximum and the "
                    "threshold run on the host inside msorb_kf_database_query (a two-launch variant was not built, so there is no A/B)",
           "box": box(), "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
