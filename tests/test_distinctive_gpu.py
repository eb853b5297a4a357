"""GPU: msorb_distinctive_descriptors on the edge sets of distinctive_cases.py against the plain reference and the oracle."""
import pytest

import distinctive_cases as dc

pytestmark = pytest.mark.gpu

SETS = dc.edge_sets()


@pytest.mark.parametrize("name", list(SETS))
def test_device_equals_reference_and_oracle(msorb_mod, oracle, name):
    desc, ob = SETS[name]
    gi, gm, _ = msorb_mod.distinctive_descriptors(desc, ob)
    ri, rm = dc.reference_distinctive(desc, ob)
    oi, om = oracle.distinctive_descriptors(desc, ob)
    same = lambda a, b, c, d: a.tolist() == c.tolist() and b.tolist() == d.tolist()
    verdict = dict(device_vs_reference=same(gi, gm, ri, rm), device_vs_oracle=same(gi, gm, oi, om), oracle_vs_reference=same(oi, om, ri, rm))
    assert all(verdict.values()), (name, verdict, [(p, int(gi[p]), int(ri[p]), int(gm[p]), int(rm[p]))
                                                   for p in range(len(ri)) if gi[p] != ri[p] or gm[p] != rm[p]][:10])


def test_size_1000_is_repeatable(msorb_mod):
    desc, ob = SETS["sweep_pool3"]
    assert ob[-1] - ob[-2] == 1000
    a = msorb_mod.distinctive_descriptors(desc, ob)
    b = msorb_mod.distinctive_descriptors(desc, ob)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
