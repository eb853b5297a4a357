"""glibc_logf AS THE DEVICE COMPILES IT (csrc/logf_restated.h inside frustum_point), every bit of it, against the installed libm:
the predicted level of msorb_is_in_frustum is made to BE the logarithm (tests/boundary_cases.py readout_groups), at every float
around every flip point of the level, over a sweep of the ratios tracking sees and over the rest of the float range; then the
same ratios at the product's own scale factor through both kernels that call frustum_point."""
import numpy as np
import pytest

import boundary_cases as bc
import track_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def logf_set(oracle):
    c = bc.logf_cases(oracle)
    return c, bc.logf_points(c["ratio"], c["kexp"])


def test_device_logf_read_out_through_the_level(msorb_mod, oracle, logf_set):
    c, (P, N, maxd, mind) = logf_set
    wrong, total, worst = 0, 0, 0
    for lsf, idx, want in bc.readout_groups(oracle, c["ratio"]):
        F = bc.frustum(lsf, bc.READOUT_LEVELS)
        a = msorb_mod.is_in_frustum(F, P[idx], N[idx], maxd[idx], mind[idx])
        b = oracle.is_in_frustum(F, P[idx], N[idx], maxd[idx], mind[idx])
        assert np.array_equal(b["level"], want) and b["track_in_view"].all()          # the read-out holds on the reference
        d = np.abs(a["level"].astype(np.int64) - want)
        wrong += int((d != 0).sum()); total += len(idx); worst = max(worst, int(d.max()))
        bad = np.nonzero(d)[0][:5]
        assert len(bad) == 0, (f"log_scale_factor {lsf}: device logf differs from libm at ratios {c['ratio'][idx][bad].tolist()} "
                               f"(depth 2^{c['kexp'][idx][bad].tolist()}) by {d[bad].tolist()} ulps")
        for k in bc.FRUSTUM_KEYS:
            assert bc.same_bits(a[k], b[k]), (lsf, k)
    print(f"device logf: {total} ratios, {wrong} differ from libm, worst {worst} ulps")
    assert total == len(c["ratio"])


@pytest.mark.parametrize("lsf", bc.log_scale_factors()[:2], ids=["logf_1.2f", "one_ulp_above"])
def test_predicted_level_at_the_product_scale(msorb_mod, oracle, logf_set, lsf):
    """the real quantity — the clamped level of an 8-level pyramid — from frustum_kernel and from local_points_kernel"""
    c, (P, N, maxd, mind) = logf_set
    F = bc.frustum(lsf, bc.NLEVELS)
    b = oracle.is_in_frustum(F, P, N, maxd, mind)
    a = msorb_mod.is_in_frustum(F, P, N, maxd, mind)
    print(f"frustum_kernel, log_scale_factor {lsf}: {int((a['level'] != b['level']).sum())} of {len(maxd)} levels differ")
    for k in bc.FRUSTUM_KEYS:
        assert bc.same_bits(a[k], b[k]), k
    kps, kdesc = bc.minimal_frame()
    mp = bc.local_points_table(P, N, maxd, mind)
    f = msorb_mod.Frame(kps, kdesc, None, bc.CAM["bounds"], bc.SCALE)
    rf = oracle.OracleFrame(kps, kdesc, None, bc.CAM["bounds"], bc.SCALE)
    try:
        fa, fb = np.full(1, -1, np.int32), np.full(1, -1, np.int32)
        nm, out = msorb_mod.search_local_points(f, F, mp, fa, 1.0)
        rnm, r, _ = tc.oracle_local_points(oracle, rf, F, mp, fb, 1.0)
        print(f"local_points_kernel, log_scale_factor {lsf}: {int((out['level'] != r['level']).sum())} of {len(maxd)} levels differ")
        for k in bc.FRUSTUM_KEYS:
            assert bc.same_bits(out[k], r[k]), k
        assert nm == rnm == 0 and np.array_equal(fa, fb)
    finally:
        f.close()
