"""msorb_mlpnp_ransac_batch on the device against R64 of tests/mlpnp_cases.py: every hypothesis' pose (hyp_pose_out) within 16 D,
hyp_flags_out, all counts, the winner record and the mask equal; the bits of Tcw are the narrowed R, t; a batch of three unequal
problems equals the single calls bit for bit; repeated calls give equal bits; every refused argument leaves every output
untouched.  D and the margin of 16: tests/test_mlpnp_host.py.  Shapes at the edges of mlpnp_hypotheses_kernel (one wavefront per
hypothesis, one ballot word per 64 correspondences): n = 6, 7, 63 / 64 / 65, 257; H = 1, 35 and 300."""
import numpy as np
import pytest

import mlpnp_cases as mc

pytestmark = pytest.mark.gpu


def test_no_named_edge_scene_is_left_out():
    assert set(mc.EDGE) <= set(mc.admitted())


@pytest.mark.parametrize("name", mc.admitted())      # a scene on which the variants of the restatement disagree decides nothing
def test_device_against_r64(msorb_mod, name):
    sc, ref = mc.prepared(name)
    bound = 16 * mc.load_spread()
    dev = msorb_mod.mlpnp_ransac_batch([mc.problem_of(sc)])[0]
    d, _ = mc.pose_difference(dev["poses"], ref["poses"])
    print(f"{name}: pose difference {d:.3e} (bound {bound:.3e}) bit_equal={dev['poses'].tobytes() == ref['poses'].tobytes()}")
    assert mc.same(dev, ref, bound) is None, mc.same(dev, ref, bound)
    again = msorb_mod.mlpnp_ransac_batch([mc.problem_of(sc)])[0]
    assert mc.same_bits(dev, again)


def test_batch_equals_the_single_calls(msorb_mod):
    scs = [mc.prepared(k)[0] for k in mc.BATCH]
    assert len({(len(sc["p2d"]), len(sc["sets"])) for sc in scs}) == 3
    batch, ms = msorb_mod.mlpnp_ransac_batch([mc.problem_of(sc) for sc in scs], timing=True)
    assert ms > 0 and len(batch) == 3
    bound = 16 * mc.load_spread()
    for k, sc, b in zip(mc.BATCH, scs, batch):
        assert mc.same(b, mc.prepared(k)[1], bound) is None, (k, mc.same(b, mc.prepared(k)[1], bound))
        assert mc.same_bits(b, msorb_mod.mlpnp_ransac_batch([mc.problem_of(sc)])[0]), k
    again = msorb_mod.mlpnp_ransac_batch([mc.problem_of(sc) for sc in scs])
    assert all(mc.same_bits(a, b) for a, b in zip(batch, again))


def test_bad_arguments_are_refused_and_nothing_is_written(msorb_mod):
    sc, ref = mc.prepared("n=150,H=1")
    n = len(sc["p2d"])
    E = msorb_mod.E_INVALID

    def call(**kw):
        return mc.raw_call(msorb_mod, sc, **kw)

    assert call(n=5, sets=[[0, 1, 2, 3, 4, 0]]) == (E, True)            # n < 6
    assert call(n_hyp=0, hyp=(0, 0)) == (E, True)                       # H < 1
    assert call(corr=(0, n - 1)) == (E, True)                           # offsets that do not match
    assert call(hyp=(0, 2)) == (E, True)
    assert call(corr=(1, n + 1)) == (E, True)
    assert call(sets=[[4, 9, 1, 2, 3, 4]]) == (E, True)                 # a repeated index
    assert call(sets=[[0, 1, 2, 3, 4, n]]) == (E, True)                 # an index >= n
    assert call(sets=[[0, 1, 2, -1, 4, 5]]) == (E, True)
    for k in ("problems", "corr", "hyp", "p2d", "p3d", "err", "sets", "inl", "res"):
        assert call(null=(k,)) == (E, True), k
    assert call(n_problems=-1) == (E, True)
    assert call(n_problems=0)[0] == msorb_mod.OK                        # nothing to do (*elapsed_ms = 0)
    assert call(null=("counts", "poses", "flags", "ms")) == (msorb_mod.OK, False)     # the optional outputs
    assert call() == (msorb_mod.OK, False)
    bound = 16 * mc.load_spread()
    assert mc.same(msorb_mod.mlpnp_ransac_batch([mc.problem_of(sc)])[0], ref, bound) is None      # and the entry still answers
