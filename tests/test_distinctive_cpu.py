"""ComputeDistinctiveDescriptors: the C++ oracle against the plain reference of distinctive_cases.py, and what the edge sets contain."""
import numpy as np
import pytest

import bow_cases
import distinctive_cases as dc

SETS = dc.edge_sets()


@pytest.mark.parametrize("name", list(SETS))
def test_oracle_equals_plain_reference(oracle, name):
    desc, ob = SETS[name]
    oi, om = oracle.distinctive_descriptors(desc, ob)
    ri, rm = dc.reference_distinctive(desc, ob)
    assert oi.tolist() == ri.tolist() and om.tolist() == rm.tolist()


def test_oracle_equals_plain_reference_on_random_descriptors(oracle):
    rng = np.random.default_rng(0)                               # the set of test_bow_gpu.py, fewer points
    sizes = [0, 1, 2, 3, 8, 9, 16, 17, 32, 33, 63, 64, 65, 130, 300] + rng.integers(0, 40, 300).tolist()
    desc, ob = bow_cases.make_observations(7, sizes)
    oi, om = oracle.distinctive_descriptors(desc, ob)
    ri, rm = dc.reference_distinctive(desc, ob)
    assert oi.tolist() == ri.tolist() and om.tolist() == rm.tolist()


def _points(name):
    desc, ob = SETS[name]
    return [desc[ob[p]:ob[p + 1]] for p in range(len(ob) - 1)]


def test_the_sweeps_hold_every_size():
    for fam in dc.FAMILIES:
        assert [len(x) for x in _points("sweep_" + fam)] == list(dc.SIZES)


def test_identical_rows_all_tie_at_zero():
    for x in _points("sweep_identical"):
        assert not dc.row_medians(x).any()
    bi, bm = dc.reference_distinctive(*SETS["sweep_identical"])
    assert not bi.any() and not bm.any()


def test_pool3_has_tied_minima_away_from_row_0():
    bi, bm = dc.reference_distinctive(*SETS["sweep_pool3"])
    tied = later = 0
    for x, i, m in zip(_points("sweep_pool3"), bi, bm):
        med = dc.row_medians(x)
        at = np.nonzero(med == med.min())[0]
        assert at[0] == i and med.min() == m
        tied += len(at) > 1
        later += i > 0 and len(at) > 1                           # the minimum is not at row 0 and occurs again behind its first row
        assert len(x) < 3 or len(np.unique(med)) > 1
    assert tied >= 17 and later >= 15


def test_complement_rows_have_median_256():
    bi, _ = dc.reference_distinctive(*SETS["sweep_complement"])
    for x, i in zip(_points("sweep_complement"), bi):
        med, N = dc.row_medians(x), len(x)
        assert set(med.tolist()) <= {0, 256}
        if N >= 3:                                               # odd and even N: the rows in front are at 256, the winner follows them
            assert (med[:(N - 1) // 2] == 256).all() and (med[(N - 1) // 2:] == 0).all() and i == (N - 1) // 2 > 0
    sizes = [len(x) for x in _points("sweep_complement") if (dc.row_medians(x) == 256).any()]
    assert any(n % 2 for n in sizes) and any(n % 2 == 0 for n in sizes) and max(sizes) == 1000 and 65 in sizes


def test_outlier_moves_the_winner_off_row_0():
    bi, _ = dc.reference_distinctive(*SETS["sweep_outlier"])
    for x, i in zip(_points("sweep_outlier"), bi):
        N = len(x)
        assert i == (1 if N % 2 and N >= 3 else 0)
        assert N < 3 or sorted(set(dc.row_medians(x).tolist())) == [0, 77]


@pytest.mark.parametrize("W", dc.WIDTHS)
def test_mixed_segments_leave_one_live_segment_in_the_last_block(W):
    sizes = [len(x) for x in _points("mixed_%d" % W)]
    per_block = dc.BLOCK // W
    assert len(sizes) % per_block == 1 and len(sizes) > per_block
    assert all((W // 2 < n <= W) or (W == 8 and 1 <= n <= 8) for n in sizes)          # all of one width class
    assert min(sizes) == (1 if W == 8 else W // 2 + 1) and max(sizes) == W
    per_wave = max(64 // W, 1)
    if per_wave > 1:                                                                   # the segments of a wavefront differ in N
        assert all(len(set(sizes[i:i + per_wave])) > 1 for i in range(0, len(sizes) - per_wave, per_wave))


def test_offset_and_empty_points():
    desc, ob = SETS["offset_begin"]
    assert ob[0] == 5
    desc, ob = SETS["empties_interleaved"]
    n = np.diff(ob)
    assert ob[0] == 3 and n[0] == 0 and (n[2::2] == 0).all() and (n[1::2] > 0).all() and n.max() > 64
    bi, bm = dc.reference_distinctive(desc, ob)
    assert (bi[n == 0] == -1).all() and (bm[n == 0] == dc.INT_MAX).all() and (bi[n > 0] >= 0).all()
