"""msorb_sim3_ransac_batch on the device against R32 of tests/sim3_cases.py: the count of every hypothesis, winner, converged,
consumed, the winner's mask and n_inliers equal; s, R, t, T12 bit-equal where R32's are finite and non-finite where they are not.
No tolerance: the kernel's float operations are the fixed ones of csrc/sim3_device.h, none contracted, and the reductions are
integer.  Shapes at the edges of sim3_hypotheses_kernel (256 threads, wavefronts of 64, one ballot word per 64 correspondences):
n = 3, 63 / 64 / 65, 255 / 256 / 257, 1025; H = 1 and 300."""
import numpy as np
import pytest

import sim3_cases as s3

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            sc = s3.SCENES[name]()
            cache[name] = (sc, s3.R32(sc))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(s3.SCENES))
def test_device_equals_r32(msorb_mod, cases, name):
    sc, ref = cases(name)
    dev = msorb_mod.sim3_ransac_batch([s3.problem_of(sc)])[0]
    assert s3.same(dev, ref) is None, s3.same(dev, ref)
    again = msorb_mod.sim3_ransac_batch([s3.problem_of(sc)])[0]
    assert s3.same_bits(dev, again)


def test_batch_equals_the_single_calls(msorb_mod, cases):
    scs = [cases(k)[0] for k in s3.BATCH]
    batch, ms = msorb_mod.sim3_ransac_batch([s3.problem_of(sc) for sc in scs], timing=True)
    assert ms > 0 and len(batch) == 3
    for k, sc, b in zip(s3.BATCH, scs, batch):
        assert s3.same(b, cases(k)[1]) is None, (k, s3.same(b, cases(k)[1]))
        assert s3.same_bits(b, msorb_mod.sim3_ransac_batch([s3.problem_of(sc)])[0]), k
    again = msorb_mod.sim3_ransac_batch([s3.problem_of(sc) for sc in scs])
    assert all(s3.same_bits(a, b) for a, b in zip(batch, again))


def test_a_carried_best_changes_the_selection_only(msorb_mod, cases):
    """the same hypotheses under another best_inliers_in / min_inliers: equal counts, the selection of the literal loop"""
    sc, ref = cases("exhausted")
    for best_in, min_inliers in ((0, 10), (int(ref["counts"].max()), 80), (int(ref["counts"].max()) + 1, 80)):
        sc2 = dict(sc, best_inliers_in=best_in, min_inliers=min_inliers)
        dev = msorb_mod.sim3_ransac_batch([s3.problem_of(sc2)])[0]
        assert s3.same(dev, s3.R32(sc2)) is None, (best_in, min_inliers)


def test_bad_arguments_are_refused_and_nothing_is_written(msorb_mod, cases):
    sc, ref = cases("H=1")
    n = len(sc["X1"])
    E = msorb_mod.E_INVALID

    def call(**kw):
        return s3.raw_call(msorb_mod, sc, **kw)

    assert call(n=2, triples=[[0, 1, 0]]) == (E, True)                   # n < 3
    assert call(n_hyp=0, hyp=(0, 0)) == (E, True)                        # H < 1
    assert call(triples=[[4, 9, 4]]) == (E, True)                        # a repeated index
    assert call(triples=[[0, 1, n]]) == (E, True)                        # an index >= n
    for k in ("problems", "corr", "hyp", "X1", "X2", "e1", "e2", "triples", "inl", "res"):
        assert call(null=(k,)) == (E, True), k
    assert call(null=("counts", "ms")) == (msorb_mod.OK, False)          # the two optional outputs
    assert call() == (msorb_mod.OK, False)
    assert s3.same(msorb_mod.sim3_ransac_batch([s3.problem_of(sc)])[0], ref) is None      # and the entry still answers
