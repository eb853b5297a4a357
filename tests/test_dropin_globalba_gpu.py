"""ms-slam_amd/host/Optimizer_device.h's BundleAdjustment / GlobalBundleAdjustemnt compiled against stand-in KeyFrame / MapPoint /
Map types (tests/dropin_globalba_main.cc), linked to libmsorb.so through the C ABI and run on the GPU.  The program makes its own
small map and checks, against msorb_bundle_adjustment on the arrays listed beside it: both write-back branches (SetPose /
SetWorldPos / UpdateNormalAndDepth, and mTcwGBA / mPosGBA / mnBAGlobalForKF), bad KeyFrames and bad points skipped, a KeyFrame
with mnId > maxKFid skipped, an edge-less point untouched, `false` with nothing touched for mpCamera2 and for more free KeyFrames
than the capacity, and the stop flag through the bool*."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_host_template(tmp_path):
    exe = tmp_path / "dropin_globalba"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include",
                           f"{ROOT}/tests/dropin_globalba_main.cc", f"-L{ROOT}/ms-slam_amd", "-lmsorb", f"-Wl,-rpath,{ROOT}/ms-slam_amd",
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok"
