#!/usr/bin/env python3
"""In-process A/B of the level-0 input paths (host-memory admission, include/msorb.h): ONE process, one extractor handle per
setting (as tools/ab_handles.py: two processes of one build differ by up to 6 % in per-frame medians), alternating blocks of 100
KITTI-sized frames, order reversed every round; per setting and entry the median of each block, the median over blocks and the
spread between blocks (max - min of the block medians).

Settings
    direct          images in msorb.host_empty arrays with 64-byte aligned rows (row stride 1280)
    direct_1241     images in contiguous msorb.host_empty arrays: row stride 1241, every row at another alignment
    staged_same     MSORB_INPUT_DIRECT=0 on the arrays of direct_1241 (the staged path fed from pinned memory)
    pageable        ordinary numpy arrays (what bench.py's per-frame legs pass)
Entries: msorb_extract, msorb_extract_stereo, msorb_track_frontend_motion, each through prepared ctypes arguments.

    python tools/input_admission_ab.py [--rounds 12] [--only pageable] [--tag NAME] [--out profiles/input_admission_ab.json]

--only pageable runs that setting alone: MSORB_LIB=<another build's libmsorb.so> --abi <its version> then measures the staged
path of that build (a library without the admission entries is driven through the entries it has).  Results are merged into --out under --tag."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd")]
import msorb  # noqa: E402
from msorb import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=12)
ap.add_argument("--block", type=int, default=100)
ap.add_argument("--only", default="")
ap.add_argument("--tag", default="run")
ap.add_argument("--abi", type=int, default=0, help="ABI version the loaded library reports, when MSORB_LIB names an older build")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_admission_ab.json"))
args = ap.parse_args()

if args.abi:
    msorb.ABI_VERSION = args.abi   # (before the library is loaded: the mirror refuses a library older than itself)
MBF = 386.1448
MB = MBF / 718.856
cfg = synth.KITTI
rows, cols = cfg["rows"], cfg["cols"]
Lp, Rp = synth.stereo_pair(0, rows, cols)
has_admission = hasattr(msorb.lib(), "msorb_host_alloc")
SETTINGS = ["direct", "direct_1241", "staged_same", "pageable"] if has_admission else ["pageable"]
if args.only:
    SETTINGS = [s for s in args.only.split(",") if s in SETTINGS]
    assert SETTINGS, "nothing to run"


def pinned(img, stride):
    block = msorb.host_empty((rows, stride))
    block[:, :cols] = img
    return block[:, :cols]


shared_1241 = (pinned(Lp, cols), pinned(Rp, cols)) if has_admission else None
ref_ex = msorb.ORBextractor(cfg["nfeatures"], cfg["scale"], cfg["nlevels"], cfg["ini_th"], cfg["min_th"])
kl, dl, kr, dr, ur, dp, oob = ref_ex.extract_stereo(Lp, Rp, MB, MBF)   # the reference result, on a handle that is not timed
ref_ex.close()
rigs = []
for name in SETTINGS:
    env = {"MSORB_INPUT_DIRECT": "0"} if name == "staged_same" else {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    ex = msorb.ORBextractor(cfg["nfeatures"], cfg["scale"], cfg["nlevels"], cfg["ini_th"], cfg["min_th"])
    for k, v in old.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    if name == "direct":
        left, right = pinned(Lp, 1280), pinned(Rp, 1280)
    elif name in ("direct_1241", "staged_same"):
        left, right = shared_1241
    else:
        left, right = Lp.copy(), Rp.copy()
    cam = synth.KITTI_CAM
    last, q, t, fw, bw = synth.last_frame(9500, kl, dl, dp)
    mm = msorb.MotionModel.make(q, t, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"], fw, bw)
    run = msorb.MotionFrontendRunner(ex, Lp, Rp, MB, MBF, mm, last, last["obs"], 7.0)
    vp = C.c_void_p
    pl, pr = vp(left.ctypes.data), vp(right.ctypes.data)
    sl, sr = left.strides[0], right.strides[0]
    s = list(run._stereo)
    s[2], s[3], s[6], s[7] = pl, pr, sl, sr   # the runner's prepared arguments, on this setting's images
    run._stereo = tuple(s)
    cap = ex.capacity
    n1, m1 = C.c_int(0), C.c_int(0)
    one_args = (ex.h, pl, rows, cols, sl, 0, 0, msorb._np_ptr(run.kl), msorb._np_ptr(run.dl), cap, C.byref(n1), C.byref(m1))
    lib = ex.L
    lib.msorb_extract_stereo.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_float, C.c_float] + [vp] * 6 + [C.c_int] + [vp] * 3
    st_args = (ex.h, pl, pr, rows, cols, sl, sr, MB, MBF) + run._stereo[10:20]
    calls = {
        "msorb_extract": lambda lib=lib, a=one_args: msorb._check(lib.msorb_extract(*a), "msorb_extract"),
        "msorb_extract_stereo": lambda lib=lib, a=st_args: msorb._check(lib.msorb_extract_stereo(*a), "msorb_extract_stereo"),
        "msorb_track_frontend_motion": run.one_call,
    }
    for fn in calls.values():
        for _ in range(30):
            fn()
    calls["msorb_extract_stereo"]()
    n = run.nl.value
    got = (run.kl[:n].copy(), run.dl[:n].copy(), run.ur[:n].copy(), run.dp[:n].copy())
    for a, b in zip(got, (kl, dl, ur, dp)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name}: results differ from the pageable call"
    rigs.append(dict(name=name, ex=ex, run=run, keep=(left, right), calls=calls, blocks={k: [] for k in calls}))

for rnd in range(args.rounds):
    for r in (rigs if rnd % 2 == 0 else rigs[::-1]):
        for entry, fn in r["calls"].items():
            for _ in range(5):
                fn()
            ts = []
            for _ in range(args.block):
                t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
            r["blocks"][entry].append(float(np.median(ts)) * 1e3)

result = dict(block_frames=args.block, rounds=args.rounds, lib=os.path.basename(os.path.dirname(msorb.LIB_PATH)) + "/" + os.path.basename(msorb.LIB_PATH),
              abi=int(msorb.lib().msorb_abi_version()), settings={})
for r in rigs:
    ent = {}
    for entry, b in r["blocks"].items():
        ent[entry] = dict(median_ms=round(float(np.median(b)), 4), spread_ms=round(max(b) - min(b), 4), block_medians_ms=[round(x, 4) for x in b])
    stats = r["ex"].input_stats() if has_admission else None
    result["settings"][r["name"]] = dict(entries=ent, input_stats=stats)
    print(f"{r['name']:12s} " + " | ".join(f"{e} {v['median_ms']:.4f} (spread {v['spread_ms']:.4f})" for e, v in ent.items()) + f"  {stats}", flush=True)
if {"direct", "direct_1241", "staged_same"} <= set(result["settings"]):
    gate = {}
    for entry in ("msorb_extract", "msorb_extract_stereo", "msorb_track_frontend_motion"):
        s_ = result["settings"]
        base = s_["staged_same"]["entries"][entry]
        for d in ("direct", "direct_1241"):
            e = s_[d]["entries"][entry]
            gap = base["median_ms"] - e["median_ms"]
            gate[f"{entry}:{d}"] = dict(gap_ms=round(gap, 4), spread_ms=max(base["spread_ms"], e["spread_ms"]), faster_beyond_spread=bool(gap > max(base["spread_ms"], e["spread_ms"])))
    result["direct_vs_staged_same"] = gate
    print(json.dumps(gate, indent=1))
doc = {}
if os.path.exists(args.out):
    with open(args.out) as f:
        doc = json.load(f)
doc[args.tag] = result
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
for r in rigs:
    r["run"].close()
    r["ex"].close()
