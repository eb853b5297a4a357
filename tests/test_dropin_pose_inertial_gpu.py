"""ms-slam_amd/host/Optimizer_device.h's PoseInertialOptimizationLastKeyFrame / LastFrame templates compiled against stand-in
Frame / KeyFrame / MapPoint / IMU::Preintegrated / IMU::Bias / ConstraintPoseImu types with the reference's member names
(tests/dropin_pose_inertial_main.cc), linked to libmsorb.so through the C ABI and run on the GPU over scenes of
tests/pose_inertial_cases.py.  The program checks every side effect against msorb_pose_inertial_optimization_batch on a problem it
gathers beside the templates, the resident-handle overloads against the flat ones, and -1 with nothing touched for the frames the
templates do not handle; see the head of the program."""
import os
import subprocess

import pytest

import pose_inertial_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_host_templates(tmp_path):
    exe = tmp_path / "dropin_pose_inertial"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include",
                           f"{ROOT}/tests/dropin_pose_inertial_main.cc", f"-L{ROOT}/ms-slam_amd", "-lmsorb", f"-Wl,-rpath,{ROOT}/ms-slam_amd",
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    names = ("mixed/0", "mixed/1", "n0/0", "n0/1", "n29_recover/1", "n29_recover_recinit/0", "close_points/0", "n257/1")
    pc.write_dropin_scenes(str(tmp_path / "in.bin"), [pc.scene(n) for n in names])
    p = subprocess.run([str(exe), str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr[-2000:])
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok"
