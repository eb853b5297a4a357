"""The shared Lie-group primitives of the optimisers ALONE on the device (msorb_debug_lie: the functions of se3_device.h,
sim3_opt_device.h, essential_graph_device.h, essential_graph4_device.h, inertial_device.h and mlpnp_device.h as hipcc compiles them
with the library's flags, against OCML), one test per function over every record of tests/lie_primitives_cases.py:

 - a function, or an arm, with no libm call other than sqrt: byte-equal to the host program (tests/lie_probe_main.cc, the same text
   through g++ and glibc);
 - everything else: within 16 D(function, family) of the exact value (the reference's formula in mpmath), D measured on the CPU
   from the float variants and kept in tests/golden/lie_primitives_sensitivity.json; where the exact value is NaN or +-inf the
   device's is the same class at the same position.
Every test prints the largest distance / D and the number of records that are not byte-equal to the host program (and the largest
distance / D among those: the libm's own share)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lie_primitives_cases as lc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("lie_primitives_gpu")
    exe = str(d / "lie_probe_main")
    b = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", os.path.join(ROOT, "tests", "lie_probe_main.cc"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    blocks = [(fn, lc.records(fn)[0]) for fn in lc.OPS]
    lc.write_blocks(str(d / "in.bin"), blocks)
    p = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-3000:])
    return dict(zip(lc.OPS, lc.read_blocks(str(d / "out.bin"), blocks)))


def test_the_python_mirror_names_the_same_operations(msorb_mod):
    assert msorb_mod.LIE_OPS == lc.OPS and (msorb_mod.LIE_IN, msorb_mod.LIE_OUT) == (lc.LIE_IN, lc.LIE_OUT)
    assert all(msorb_mod.lie_in_width(i) == lc.in_width(fn) for i, fn in enumerate(lc.OPS))


@pytest.mark.parametrize("fn", lc.OPS)
def test_the_device_against_the_host_program_and_the_exact_value(fn, msorb_mod, host_outputs):
    rec = lc.records(fn)[0]
    dev = msorb_mod.debug_lie(fn, rec)
    worst, worst_differing, differ, failures = lc.judge(fn, dev, host_outputs[fn])
    print(f"{fn}: {len(rec)} records, device: largest distance / D {worst:.3f}, not byte-equal to the host program {differ}"
          f" (largest distance / D among those {worst_differing:.3f})")
    assert not failures, (len(failures), failures[:5])


@pytest.mark.parametrize("fn", ("se3_exp", "bias_corrected"))
def test_sizes_and_arguments(fn, msorb_mod, host_outputs):
    rec = lc.records(fn)[0]
    full = msorb_mod.debug_lie(fn, np.resize(rec, (257, rec.shape[1])))
    again = msorb_mod.debug_lie(fn, np.resize(rec, (257, rec.shape[1])))
    assert full.tobytes() == again.tobytes()                       # two calls, the same bits
    for n in (1, 255, 256):                                        # a launch of one block, full or not, and of two
        part = msorb_mod.debug_lie(fn, np.resize(rec, (257, rec.shape[1]))[:n])
        assert part.shape == (n, lc.LIE_OUT) and part.tobytes() == full[:n].tobytes(), n
    assert msorb_mod.debug_lie(fn, np.zeros((0, rec.shape[1]))).shape == (0, lc.LIE_OUT)
    L = msorb_mod.lib()
    L.msorb_debug_lie.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    op = lc.OPS.index(fn)
    assert L.msorb_debug_lie(0, op, None, 0, None) == 0            # n == 0 launches nothing and reads no pointer
    one = np.ascontiguousarray(rec[:1])
    out = np.full((1, lc.LIE_OUT), 7.0)
    p_in, p_out = one.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for args in ((op, None, 1, p_out), (op, p_in, 1, None), (op, p_in, -1, p_out), (-1, p_in, 1, p_out), (len(lc.OPS), p_in, 1, p_out)):
        assert L.msorb_debug_lie(0, *args) == msorb_mod.E_INVALID, args[2]
        assert np.all(out == 7.0)                                  # a refusal leaves the output untouched
