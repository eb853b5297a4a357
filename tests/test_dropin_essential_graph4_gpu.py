"""ms-slam_amd/host/Optimizer_device.h's OptimizeEssentialGraph4DoF compiled against stand-in KeyFrame / MapPoint / Map / SE3f /
Sim3 types (tests/dropin_essential_graph4_main.cc), linked to libmsorb.so through the C ABI and run on the GPU.  The program makes
its own map and checks, against msorb_essential_graph4 on the arrays listed beside it: every live edge arm (loop connections,
mPrevKF, older loop edges, covisibility), the dead spanning-tree arm adding nothing, the weight gate and its pCurKF / pLoopKF
exemption, sInsertedEdges, the mPrevKF / mNextKF / child / loop-edge exclusions, a bad and a null neighbour, an mPrevKF without a
vertex whose edge is not added, both vertex constructors (CorrectedSim3 with a scale that the vertex drops, and the KeyFrame's four
floats), SetPose and the point correction byte-equal to the formulas on the device's poses, a bad point untouched, and `false` with
nothing touched for a bad KeyFrame in the map, an id above GetMaxKFid() and more free KeyFrames than the capacity."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_host_template(tmp_path):
    exe = tmp_path / "dropin_essential_graph4"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include",
                           f"{ROOT}/tests/dropin_essential_graph4_main.cc", f"-L{ROOT}/ms-slam_amd", "-lmsorb", f"-Wl,-rpath,{ROOT}/ms-slam_amd",
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok"
