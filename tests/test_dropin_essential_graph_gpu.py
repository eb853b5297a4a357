"""ms-slam_amd/host/Optimizer_device.h's two OptimizeEssentialGraph overloads compiled against stand-in KeyFrame / MapPoint / Map /
SE3f / Sim3 types (tests/dropin_essential_graph_main.cc), linked to libmsorb.so through the C ABI and run on the GPU.  The program
makes its own maps and checks, against msorb_essential_graph on the arrays listed beside them.  Loop closing, with fixed and with
free scale: every edge arm (loop connections, spanning tree, older loop edges, covisibility, inertial), the weight gate and its
pCurKF / pLoopKF exemption, sInsertedEdges, a child, a bad and a null neighbour, an edge to a KeyFrame without a vertex that is not
added, the CorrectedSim3 / NonCorrectedSim3 look-ups, SetPose with t / s, the point correction through both reference-KeyFrame
arms and through an id without a vertex (the identity), a bad point untouched, and `false` with nothing touched for a bad KeyFrame
in the map and above the capacity.  Merging: the three classes with per-vertex fix_scale, a KeyFrame in two lists, a bad one, the
vpGoodPose / vpBadPose relations of the three arms, the BefMerge fields and SetPose, the float point loop with its
EraseObservation walk and the "another map" arm, and `false` with nothing touched above the capacity."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_host_template(tmp_path):
    exe = tmp_path / "dropin_essential_graph"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include",
                           f"{ROOT}/tests/dropin_essential_graph_main.cc", f"-L{ROOT}/ms-slam_amd", "-lmsorb", f"-Wl,-rpath,{ROOT}/ms-slam_amd",
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok"
