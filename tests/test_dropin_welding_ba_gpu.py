"""ms-slam_amd/host/Optimizer_device.h's welding LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag) compiled against
stand-in KeyFrame / MapPoint / Map types (tests/dropin_welding_ba_main.cc).

CPU: the gathering walk (:3515-3707) and the stop-flag mirror alone, built WITHOUT the library as a stand-alone program, plain and
under ASan + UBSan: the gathered arrays equal the arrays listed by hand beside the map (fixed KeyFrames first, the points in the
order of the walk, the mnBALocalForMerge marks, a bad KeyFrame, a KeyFrame and a point of another map, a KeyFrame in no list, a bad
point, octave 11 and an empty slot all dropped), restore_marks puts every mark back, and a bool set by another thread reaches the
int the C ABI reads.

GPU: the whole template, linked to libmsorb.so.  Against msorb_welding_ba on the listed arrays: SetPose on the adjustable
KeyFrames alone and SetWorldPos + UpdateNormalAndDepth on every gathered point with the returned bits, the erased observations
are exactly the flagged edges (both sides of each), a stop flag that stays clear changes nothing, one that is set returns true
with the marks alone, one raised between the rounds through the library's poll hook gives status 3 with round 1's estimates and
flags, and `false` with every mark put back for a camera that is no pinhole and for more adjustable KeyFrames than the capacity."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = f"{ROOT}/tests/dropin_welding_ba_main.cc"
INC = [f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include"]


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_the_gathering_and_the_stop_flag_mirror_without_the_library(tmp_path, sanitize):
    exe = str(tmp_path / "dropin_welding_ba_gather")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", "-pthread", "-DWELDING_BA_GATHER_ONLY",
                        *sanitize, *INC, SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    p = subprocess.run([exe, "--gather"], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok"


@pytest.mark.gpu
def test_host_template(tmp_path):
    exe = tmp_path / "dropin_welding_ba"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", *INC, SRC, f"-L{ROOT}/ms-slam_amd", "-lmsorb",
                           f"-Wl,-rpath,{ROOT}/ms-slam_amd", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok"
