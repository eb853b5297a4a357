#!/usr/bin/env python3
"""Latency of msorb_create_new_map_points_kf against the exact alternative of the commit before it, through the Python mirror.

Per K in (10, 20, 30) neighbours of n = 2000 features each (tests/new_map_points_cases.make_scene):
  new       one KeyFrameStore.create_new_map_points call: search, triangulation and gates of all K neighbours, one round trip
  baseline  K sequential KeyFrameStore.search_for_triangulation calls of one pair each, the host clearing the queries that got a
            point in between (the points themselves taken from a run made beforehand: the host triangulation the baseline would
            need is NOT timed, which favours the baseline)
Both are timed with a host clock around calls that end in a stream synchronise, in one process, in alternating blocks after a
warm-up; the figure is the median over the blocks of a block's mean.  The device-event split of the new call (match / histogram /
new points, summed over the neighbours) comes from a child process with MSORB_NEW_POINTS_STAGES=1, because the events between the
launches are themselves work.  Writes profiles/new_map_points_latency.json.  Needs a GPU; says so and fails without one."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ms-slam_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import msorb  # noqa: E402
import new_map_points_cases as nmp  # noqa: E402


def setup(K, n):
    sc = nmp.make_scene(100 + K, n1=n, K=K, n2=n, n_nodes=100, check_orientation=False, step=(0.15, 0.01, 0.1))
    store = msorb.KeyFrameStore()
    ids = nmp.store_scene(store, sc)
    call, nbs = nmp.device_call(sc, ids)
    stereo = [(kf["geometry"]["u_right"] >= 0).astype(np.uint8) for kf in sc["kfs"]]
    pairs = [dict(kf1=ids[0], kf2=ids[k + 1], avail2=sc["avail2"][k], stereo1=stereo[0], stereo2=stereo[k + 1], F12=sc["F12"][k],
                  ep=sc["ep"][k]) for k in range(K)]
    return sc, store, call, nbs, pairs


def measure(K, n, blocks, per_block, warmup):
    sc, store, call, nbs, pairs = setup(K, n)
    first = store.create_new_map_points(call, nbs)
    made = [np.nonzero((r["status"] >= nmp.TRIANGULATED) & (r["status"] <= nmp.STEREO2))[0] for r in first]

    def new():
        return store.create_new_map_points(call, nbs, timing=True)

    def baseline():
        valid = sc["valid1"].copy()
        out, ms = [], 0.0
        for k in range(K):
            r, t = store.search_for_triangulation([dict(pairs[k], valid1=valid)], sc["coarse"], sc["check_orientation"])
            out.append(r[0][1])
            ms += t
            valid[made[k]] = 0
        return out, ms

    b = baseline()[0]
    same = all(np.array_equal(x, r["match12"]) for x, r in zip(b, first))    # the two paths find the same matches
    for _ in range(warmup):
        new()
        baseline()
    t_new, t_base, d_new, d_base = [], [], [], []
    for _ in range(blocks):
        t0 = time.perf_counter()
        dev = [new()[1] for _ in range(per_block)]
        t1 = time.perf_counter()
        devb = [baseline()[1] for _ in range(per_block)]
        t2 = time.perf_counter()
        t_new.append((t1 - t0) / per_block * 1e3)
        t_base.append((t2 - t1) / per_block * 1e3)
        d_new.append(float(np.mean(dev)))
        d_base.append(float(np.mean(devb)))
    res = dict(K=K, n=n, matches=int(sum(r["nmatches"] for r in first)), created=int(sum(r["n_created"] for r in first)),
               same_matches_as_baseline=bool(same),
               new_call_ms=float(np.median(t_new)), new_call_ms_blocks=[round(x, 4) for x in t_new],
               baseline_ms=float(np.median(t_base)), baseline_ms_blocks=[round(x, 4) for x in t_base],
               new_call_device_ms=float(np.median(d_new)), baseline_device_ms=float(np.median(d_base)))
    store.close()
    return res


def split(K, n, reps):
    _, store, call, nbs, _ = setup(K, n)
    for _ in range(5):
        store.create_new_map_points(call, nbs, timing=True)
    rows = []
    for _ in range(reps):
        store.create_new_map_points(call, nbs, timing=True)
        rows.append(msorb.new_map_points_stage_ms())
    store.close()
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--K", type=int, nargs="+", default=[10, 20, 30])
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--split", action="store_true", help="(child) print the device-event split as JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "new_map_points_latency.json"))
    a = ap.parse_args()
    if msorb.lib().msorb_device_count() <= 0:
        sys.exit("no GPU: nothing measured")
    if a.split:
        print(json.dumps({str(K): split(K, a.n, 30) for K in a.K}))
        return
    rows = [measure(K, a.n, a.blocks, a.per_block, a.warmup) for K in a.K]
    env = dict(os.environ, MSORB_NEW_POINTS_STAGES="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--split", "--n", str(a.n), "--K", *map(str, a.K)], env=env,
                           capture_output=True, text=True, timeout=600)
    if child.returncode != 0:
        sys.exit("split run failed: " + child.stderr[-2000:])
    sp = json.loads(child.stdout.strip().splitlines()[-1])
    for r in rows:
        r["device_split_ms"] = sp[str(r["K"])]
    rec = dict(what="msorb_create_new_map_points_kf against K sequential msorb_search_for_triangulation_kf calls with the host updating "
                    "the mask in between (the host triangulation of the baseline not timed); host clock, medians over blocks, MI355X",
               blocks=a.blocks, calls_per_block=a.per_block, warmup_calls=a.warmup, results=rows)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
