"""batch_compare.read_dump, which test_bench_batch_gpu.py uses to decode bench.py --dump-outputs, checked on the CPU: oracle
outputs of a few small images written by bench.dump_outputs come back bit for bit, and the per-image comparison fails when
two images' outputs are swapped or the outputs repeat with period 2 — so the comparison of the bench batch can fail."""
import os
import sys

import numpy as np
import pytest

from msorb import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from batch_compare import OracleBatch, read_dump  # noqa: E402

NFEAT, ROWS, COLS = 300, 240, 320


@pytest.fixture(scope="module")
def small(oracle):
    ex = oracle.OracleExtractor(NFEAT, 1.2, 8, 20, 7)
    imgs = [synth.stereo_pair(40 + i // 2, ROWS, COLS)[i % 2] for i in range(4)]
    ref = OracleBatch(*zip(*[ex(im, (0, COLS // 2)) for im in imgs]))
    assert ref.distinct() and all(len(k) > 100 for k in ref.kps)
    assert np.any(ref.mono != [len(k) for k in ref.kps])          # a lapping area: monoIndex is not the count
    return ref


def _dump(bench, torch, ref, order, path):
    """Write the oracle outputs of images `order` (position p holds image order[p]) as the library's (n, cap, 28) / (n, cap, 32)
    blocks, with bytes past each image's count that are not the oracle's, then read the dump back."""
    import msorb
    n, cap = len(order), NFEAT + 19 * 8
    rng = np.random.Generator(np.random.PCG64(5))
    kps = rng.integers(0, 256, (n, cap, 28), dtype=np.uint8)
    desc = rng.integers(0, 256, (n, cap, 32), dtype=np.uint8)
    counts = np.array([len(ref.kps[j]) for j in order], np.int32)
    for p, j in enumerate(order):
        kps[p, :counts[p]] = ref.kps[j].view(np.uint8).reshape(-1, 28)
        desc[p, :counts[p]] = ref.desc[j]
    bench.dump_outputs(str(path), counts, ref.mono[list(order)], torch.from_numpy(kps), torch.from_numpy(desc))
    return read_dump(str(path), msorb.KP_DTYPE)


def test_dump_round_trip_is_bit_exact_and_the_comparison_has_teeth(small, tmp_path, monkeypatch):
    import torch
    import bench
    ref = small
    counts, mono, kps, desc = _dump(bench, torch, ref, [0, 1, 2, 3], tmp_path / "same")
    ref.assert_batch(counts, mono, kps, desc)
    for j in range(4):
        assert kps[j].tobytes() == ref.kps[j].tobytes() and desc[j].tobytes() == ref.desc[j].tobytes()
    # the same outputs at other positions: wherever they sit, the comparison by position must fail
    got = _dump(bench, torch, ref, [0, 3, 2, 1], tmp_path / "swap")
    with pytest.raises(AssertionError, match=r"2 of 4 images differ.*image 1:"):
        ref.assert_batch(*got)
    ref.assert_batch(*got, src=[0, 3, 2, 1])                       # ... and pass against the permuted oracle
    got = _dump(bench, torch, ref, [0, 1, 0, 1], tmp_path / "tiled")
    with pytest.raises(AssertionError, match=r"2 of 4 images differ.*image 2"):
        ref.assert_batch(*got)
    # a dump that had to sample its rows cannot be split by image: the reader refuses it
    monkeypatch.setattr(bench, "DUMP_BUDGET", 50_000)
    with pytest.raises(AssertionError, match="sample"):
        _dump(bench, torch, ref, [0, 1, 2, 3], tmp_path / "sampled")
