"""The per-thread scratch protocol of ms-slam_amd/csrc/hip_host.h on the CPU: a thread that calls an entry with device B after device A
frees A's stream, events and blocks with A current and creates B's with B current; a failed creation leaves nothing marked valid; a
thread that exits after the runtime has shut down frees nothing; the grow-only buffers allocate count * sizeof(T) + 16 bytes.
tests/thread_scratch_main.cc, compiled with g++ against the HIP stand-in of tests/hip_stub (which aborts when an object is freed with
another device current than its own); no hipcc, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "thread_scratch_main.cc")
INCLUDES = [f"-I{ROOT}/tests/hip_stub", f"-I{ROOT}/ms-slam_amd/csrc"]


def test_thread_scratch_protocol(tmp_path):
    exe = str(tmp_path / "thread_scratch")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-D_GLIBCXX_ASSERTIONS", *INCLUDES, MAIN, "-o", exe,
                        "-pthread"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"exit status {p.returncode}\n{p.stderr[-4000:]}"
    assert p.stdout.strip() == "ok", p.stdout
