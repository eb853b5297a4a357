"""The host-memory admission table (ms-slam_amd/csrc/host_admission.h) and the pinned pool / cv::MatAllocator adaptor
(ms-slam_amd/host/PinnedMat.h) on the CPU: tests/host_admission_main.cc with malloc backends, one section per test; then what the
library's entries answer on a machine without a HIP device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-Wall", f"-I{ROOT}/tests/cv_stub_alloc", f"-I{ROOT}/tests/cv_stub", f"-I{ROOT}/ms-slam_amd/host",
         f"-I{ROOT}/ms-slam_amd/csrc", f"-I{ROOT}/include", f"{ROOT}/tests/host_admission_main.cc", "-lpthread"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("host_admission") / "host_admission_main"
    subprocess.check_call(["g++", "-O2"] + FLAGS + ["-o", str(out)])   # (the adaptor compiles against the layered stand-in)
    return str(out)


@pytest.mark.parametrize("section", ["lookup", "holds", "threads", "pool", "adaptor"])
def test_section(exe, section):
    """lookup: inside / first and last byte outside / across two adjacent entries / empty table.  holds: overlapping
    registrations refused, free of a held entry refused and fine after release.  threads: two lookup threads against an
    alloc / free thread, 20 000 iterations.  pool: reuse, no backend call on the second acquire of a class, budget trims idle
    blocks only.  adaptor: allocate / deallocate round trip through cv::Mat, requests below the threshold never reach the pool."""
    r = subprocess.run([exe, section], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"ok {section}" in r.stdout, r.stdout + r.stderr


def test_threads_under_the_thread_sanitizer(tmp_path):
    """A host-side -fsanitize=thread build of the same main, where the toolchain has the runtime."""
    out = tmp_path / "host_admission_tsan"
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    if shutil.which("g++") is None or subprocess.run(["g++", "-fsanitize=thread", str(probe), "-o", str(tmp_path / "probe")],
                                                      capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no thread sanitizer runtime")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=thread"] + FLAGS + ["-o", str(out)])
    r = subprocess.run([str(out), "threads"], capture_output=True, text=True, timeout=600)
    if "FATAL: ThreadSanitizer" in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr:
        pytest.skip("the thread sanitizer cannot map its shadow memory here: " + r.stderr.strip().splitlines()[0])
    assert r.returncode == 0 and "ok threads" in r.stdout and "WARNING: ThreadSanitizer" not in r.stderr, r.stdout + r.stderr


def test_pool_alone_needs_no_opencv(tmp_path):
    """MSORB_PINNED_POOL_ONLY: the pool without the OpenCV adaptor and without the library's header."""
    src = tmp_path / "pool_only.cc"
    src.write_text('#define MSORB_PINNED_POOL_ONLY\n#include "PinnedMat.h"\n#include <cstdlib>\n'
                   "static int a(size_t n, void** o) { *o = std::malloc(n); return 0; }\nstatic int f(void* p) { std::free(p); return 0; }\n"
                   "int main() { msorb_host::PinnedPool p(msorb_host::PinnedBackend{a, f}); void* b = p.acquire(70000);\n"
                   "  return b && p.release(b) && p.acquire(66000) == b ? 0 : 1; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", f"-I{ROOT}/ms-slam_amd/host", str(src), "-o", str(tmp_path / "pool_only")])
    assert subprocess.run([str(tmp_path / "pool_only")]).returncode == 0


def test_without_a_device_nothing_is_admitted(msorb_mod):
    L = msorb_mod._hlib()
    if L.msorb_device_count() > 0:
        pytest.skip("a GPU is present")
    p = C.c_void_p()
    assert L.msorb_host_alloc(4096, C.byref(p)) == msorb_mod.E_NO_DEVICE and not p.value
    assert b"no usable HIP device" in L.msorb_last_error()
    a = np.zeros(8192, np.uint8)
    assert L.msorb_host_register(a.ctypes.data_as(C.c_void_p), a.size) == msorb_mod.E_NO_DEVICE
    assert L.msorb_host_admitted(a.ctypes.data_as(C.c_void_p), a.size) == 0 and not msorb_mod.host_admitted(a)
    assert L.msorb_host_unregister(a.ctypes.data_as(C.c_void_p)) == msorb_mod.E_INVALID
    assert L.msorb_host_free(a.ctypes.data_as(C.c_void_p)) == msorb_mod.E_INVALID
    with pytest.raises(msorb_mod.MsorbError) as e:
        msorb_mod.host_empty((4, 4))
    assert e.value.code == msorb_mod.E_NO_DEVICE
    with pytest.raises(msorb_mod.MsorbError):
        with msorb_mod.host_registered(a):
            pass
    assert msorb_mod.ABI_VERSION == L.msorb_abi_version() == 6002
