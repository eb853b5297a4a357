"""glibc_sincosf<true> AS THE DEVICE COMPILES IT — the a = cos, b = sin describe_kernel steers the rBRIEF pattern with, seen in the
extractor only through 512 rounded tap positions — against the installed libm's cosf / sinf, bit for bit, through
msorb_debug_cos_sin (the device function describe_kernel itself calls)."""
import numpy as np
import pytest

import boundary_cases as bc

pytestmark = pytest.mark.gpu


def test_device_cos_sin_is_libm_bit_for_bit(msorb_mod, oracle):
    ang = bc.sincos_angles(oracle)
    a, b = msorb_mod.debug_cos_sin(ang)
    ra, rb = oracle.cos_sin_n(ang)
    da, db = a.view(np.uint32) != ra.view(np.uint32), b.view(np.uint32) != rb.view(np.uint32)
    print(f"device sincosf: {len(ang)} angles, cos differs at {int(da.sum())}, sin differs at {int(db.sum())}")
    bad = np.nonzero(da | db)[0][:8]
    assert len(bad) == 0, [(float(ang[i]), a[i].tobytes().hex(), ra[i].tobytes().hex(), b[i].tobytes().hex(), rb[i].tobytes().hex()) for i in bad]


def test_debug_cos_sin_sizes_and_arguments(msorb_mod, oracle):
    """one element, a partial block, a block and one more; nothing for nothing; the oracle's scalar form agrees"""
    for n in (1, 255, 256, 257):
        ang = np.linspace(0, 360, n, dtype=np.float32)
        a, b = msorb_mod.debug_cos_sin(ang)
        ra, rb = oracle.cos_sin_n(ang)
        assert a.tobytes() == ra.tobytes() and b.tobytes() == rb.tobytes(), n
    assert (float(a[-1]), float(b[-1])) == oracle.cos_sin(360.0)
    a, b = msorb_mod.debug_cos_sin(np.zeros(0, np.float32))
    assert len(a) == 0 and len(b) == 0
    L = msorb_mod.lib()
    assert L.msorb_debug_cos_sin(0, None, 4, None, None) == msorb_mod.E_INVALID
    assert L.msorb_debug_cos_sin(0, None, -1, None, None) == msorb_mod.E_INVALID
