#!/usr/bin/env python3
"""What every extractor entry gives the GPU, as an ordered list of kernel launches per call.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/extractor_launches.py run
    python tools/extractor_launches.py print DIR

`run` makes one handle per mode (default, stage timing on, one sub-batch with the blur on the main stream, each MSORB_FRAME_FUSE
value, MSORB_SERIAL_PIPELINE, MSORB_QUADTREE=host) and, for every entry the mode serves, one warm call and one traced call at the
small test geometry; a one-element msorb_debug_cos_sin launch marks both ends of the traced call.  `print` cuts the kernel trace
at those marks and prints, per traced call and per hardware queue, kernel name, grid and workgroup size in launch order (queues
are listed in the order of their text: the trace's queue ids differ from process to process).  MSORB_LIB picks the library, so
the lists of two builds can be compared with diff."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ms-slam_amd"))

CFG = dict(rows=240, cols=320, nfeatures=500)
DEVICE_PIPELINE = ("one image", "one image, host pyramid", "pair", "stereo", "batch 3", "batch 17", "submit + wait 17")
MODES = [
    ("default", {}, (), DEVICE_PIPELINE),
    ("stage timing on", {}, (("set_profiling", (True,)),), tuple(e for e in DEVICE_PIPELINE if e != "pair")),
    ("set_overlap(1, False)", {}, (("set_overlap", (1, False)),), DEVICE_PIPELINE),
    ("MSORB_FRAME_FUSE=0", {"MSORB_FRAME_FUSE": "0"}, (), DEVICE_PIPELINE),
    ("MSORB_FRAME_FUSE=1", {"MSORB_FRAME_FUSE": "1"}, (), DEVICE_PIPELINE),
    ("MSORB_FRAME_FUSE=2", {"MSORB_FRAME_FUSE": "2"}, (), DEVICE_PIPELINE),
    ("MSORB_SERIAL_PIPELINE=1", {"MSORB_SERIAL_PIPELINE": "1"}, (), ("one image", "one image, host pyramid", "batch 3", "batch 17")),
    ("MSORB_QUADTREE=host", {"MSORB_QUADTREE": "host", "MSORB_HOST_THREADS": "2"}, (), ("one image", "one image, host pyramid", "batch 3", "batch 17")),
]
MARK = "debug_cos_sin"


def calls():
    """-> [(mode, entry)] in the order `run` makes its traced calls."""
    return [(m[0], e) for m in MODES for e in m[3]]


def run():
    import numpy as np
    import torch
    import msorb
    from msorb import synth
    imgs = np.stack([synth.image(400 + i, CFG["rows"], CFG["cols"]) for i in range(17)])
    L, R = synth.stereo_pair(77, CFG["rows"], CFG["cols"])
    d3, d17 = torch.from_numpy(imgs[:3]).cuda(), torch.from_numpy(imgs).cuda()
    zero = np.zeros(1, np.float32)

    def mark():
        torch.cuda.synchronize()
        msorb.debug_cos_sin(zero)

    for name, env, setup, entries in MODES:
        os.environ.update(env)
        ex = msorb.ORBextractor(CFG["nfeatures"], 1.2, 8, 20, 7)
        for k in env:
            del os.environ[k]
        for fn, args in setup:
            getattr(ex, fn)(*args)

        def submit_wait():
            ex.extract_batch_submit(d17)
            ex.extract_batch_wait()

        def with_host_pyramid():
            ex.set_host_pyramid(True)
            ex(imgs[0])
            ex.pyramid_level(3)
            ex.set_host_pyramid(False)

        table = {"one image": lambda: ex(imgs[0]), "one image, host pyramid": with_host_pyramid, "pair": lambda: ex.extract_pair(L, R),
                 "stereo": lambda: ex.extract_stereo(L, R, 0.5, 380.0), "batch 3": lambda: ex.extract_batch(d3),
                 "batch 17": lambda: ex.extract_batch(d17), "submit + wait 17": submit_wait}
        for e in entries:
            table[e]()      # warm
            mark()
            table[e]()      # traced
            mark()
        ex.close()
    print("ok", len(calls()), "traced calls")


def show(out):
    f = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        raise SystemExit(f"no kernel trace under {out}")
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
    regions, cur = [], []
    for r in rows:
        if MARK in r["Kernel_Name"]:
            regions.append(cur)
            cur = []
        else:
            cur.append(r)
    traced = regions[1::2]          # [before the first mark = warm][traced][warm][traced]...
    want = calls()
    if len(traced) != len(want):
        raise SystemExit(f"{len(traced)} traced regions in the trace, {len(want)} calls expected")
    for (mode, entry), reg in zip(want, traced):
        print(f"== {mode} / {entry}: {len(reg)} launches")
        queues = {}
        for r in reg:
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            line = "%s grid (%s,%s,%s) workgroup (%s,%s,%s)" % (name, r.get("Grid_Size_X"), r.get("Grid_Size_Y"), r.get("Grid_Size_Z"),
                                                                r.get("Workgroup_Size_X"), r.get("Workgroup_Size_Y"), r.get("Workgroup_Size_Z"))
            queues.setdefault(r.get("Queue_Id", "?"), []).append(line)
        for i, q in enumerate(sorted(queues.values(), key=lambda q: "\n".join(q))):
            print(f"  queue {chr(ord('a') + i)}")
            for line in q:
                print("    " + line)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) > 2 and sys.argv[1] == "print":
        show(sys.argv[2])
    else:
        raise SystemExit(__doc__)
