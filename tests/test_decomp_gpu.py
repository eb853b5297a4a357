"""The small dense decompositions of the solvers and optimisers ALONE on the device (msorb_debug_decomp: the functions of
two_view_device.h, new_points_device.h, sim3_device.h, mlpnp_device.h and inertial_device.h as hipcc compiles them with the
library's flags), one test per routine over every record of tests/decomp_cases.py.  None of them calls libm beyond sqrt and
division, so every record is byte-equal to the host program (tests/decomp_probe_main.cc, the same text through g++, one lane of
one; a NaN matches a NaN at the same position), and so within 16 D of the exact value as the host program is.  The two cooperative
null vectors run as their kernels run them (a workgroup of 256 on a TvWork, of 64 on an MlpnpWork, in LDS); every lane's x is
compared with lane 0's on the device and no lane may differ.  Every test prints the number of records that are not byte-equal
(expected 0), the lanes that differed (expected 0) and the largest measure / D."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import decomp_cases as dc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("decomp_gpu")
    exe = str(d / "decomp_probe_main")
    b = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-O2", os.path.join(ROOT, "tests", "decomp_probe_main.cc"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    blocks = [(op, dc.records(op)[0]) for op in dc.OPS]
    dc.write_blocks(str(d / "in.bin"), blocks)
    p = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-3000:])
    return dict(zip(dc.OPS, dc.read_blocks(str(d / "out.bin"), blocks)))


def test_the_python_mirror_names_the_same_operations(msorb_mod):
    assert msorb_mod.DECOMP_OPS == dc.OPS and msorb_mod.DECOMP_OUT == dc.DECOMP_OUT
    assert msorb_mod.DECOMP_IN == tuple(dc.in_width(op) for op in dc.OPS) and msorb_mod.DECOMP_MISMATCH == dc.COOPERATIVE


@pytest.mark.parametrize("op", dc.OPS)
def test_the_device_against_the_host_program(op, msorb_mod, host_outputs):
    rec, fams = dc.records(op)
    dev = msorb_mod.debug_decomp(op, rec)
    differ = dc.differing_records(dev, host_outputs[op])
    lanes = int(dev[:, dc.COOPERATIVE[op]].sum()) if op in dc.COOPERATIVE else 0
    worst, failures = dc.judge(op, dev)
    print(f"{op}: {len(rec)} records, not byte-equal to the host program {len(differ)}, lanes that differ from lane 0 {lanes}, "
          f"device: largest measure / D {worst:.3f}")
    assert not differ, (len(differ), [(i, fams[i]) for i in differ[:5]])
    assert lanes == 0
    assert not failures, (len(failures), failures[:5])


@pytest.mark.parametrize("op", ("tv_svd3", "inertial_ldlt", "tv_null_vector_16", "mlpnp_null_vector_9"))
def test_sizes_and_arguments(op, msorb_mod, host_outputs):
    rec = dc.records(op)[0]
    sizes = (1, 2, 65) if op in dc.COOPERATIVE else (1, 255, 256, 257)      # workgroups for a cooperative op, threads otherwise
    big = np.resize(rec, (sizes[-1], rec.shape[1]))
    full, again = msorb_mod.debug_decomp(op, big), msorb_mod.debug_decomp(op, big)
    assert dc.same_bits(full, again)                                          # two calls, the same bits
    assert dc.same_bits(full, np.resize(host_outputs[op], (sizes[-1], dc.DECOMP_OUT)))
    for n in sizes[:-1]:
        part = msorb_mod.debug_decomp(op, big[:n])
        assert part.shape == (n, dc.DECOMP_OUT) and dc.same_bits(part, full[:n]), n
    assert msorb_mod.debug_decomp(op, np.zeros((0, rec.shape[1]))).shape == (0, dc.DECOMP_OUT)
    L = msorb_mod.lib()
    L.msorb_debug_decomp.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    k = dc.OPS.index(op)
    assert L.msorb_debug_decomp(0, k, None, 0, None) == 0                    # n == 0 launches nothing and reads no pointer
    one = np.ascontiguousarray(rec[:1])
    out = np.full((1, dc.DECOMP_OUT), 7.0)
    p_in, p_out = one.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for args in ((k, None, 1, p_out), (k, p_in, 1, None), (k, p_in, -1, p_out), (-1, p_in, 1, p_out), (len(dc.OPS), p_in, 1, p_out)):
        assert L.msorb_debug_decomp(0, *args) == msorb_mod.E_INVALID, args[2]
        assert np.all(out == 7.0)                                             # a refusal leaves the output untouched
