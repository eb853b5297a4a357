"""bench_legs.optional_leg: a parity self-check and a library / device failure always propagate, an environment failure becomes
the leg's "error" field and is listed in the line's "degraded_legs"."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_optional_leg_semantics(monkeypatch, capsys):
    import bench_legs as bl
    assert bl.optional_leg("x", lambda a, b=1: a + b, 2, b=3) == 5
    r = bl.optional_leg("boom", lambda: (_ for _ in ()).throw(FileNotFoundError("rocprofv3")))
    assert r == {"error": "FileNotFoundError: rocprofv3", "leg": "boom"}
    assert "optional leg 'boom' failed" in capsys.readouterr().err
    with pytest.raises(bl.SelfCheckError):
        bl.optional_leg("parity", lambda: bl.self_check(False, "gpu != cpu"))
    with pytest.raises(AssertionError):
        bl.optional_leg("assert", lambda: (_ for _ in ()).throw(AssertionError("x")))
    monkeypatch.setenv("MSORB_BENCH_FAIL_LEG", "forced")
    assert bl.optional_leg("forced", lambda: 1)["leg"] == "forced" and bl.optional_leg("other", lambda: 1) == 1
    assert bl.DEGRADED[-2:] == ["boom", "forced"]
    # a failure of libmsorb (an error code of a C-ABI entry) or of the device is a regression, not an environment problem: never degraded
    import msorb
    with pytest.raises(msorb.MsorbError):
        bl.optional_leg("lib", lambda: (_ for _ in ()).throw(msorb.MsorbError(-5, "msorb_extract_batch")))
    with pytest.raises(RuntimeError, match="HIP error"):
        bl.optional_leg("hip", lambda: (_ for _ in ()).throw(RuntimeError("HIP error: an illegal memory access was encountered")))
    monkeypatch.setenv("MSORB_BENCH_FAIL_LEG", "forced:library")
    with pytest.raises(RuntimeError, match="forced library failure"):
        bl.optional_leg("forced", lambda: 1)
    assert "lib" not in bl.DEGRADED and "hip" not in bl.DEGRADED


def test_every_leg_module_imports_without_a_gpu():
    import importlib
    for m in ("cpu", "density", "hamming", "host_fed", "per_frame", "pmc", "sparsification", "split", "stereo", "tracking", "unchanged"):
        importlib.import_module("bench_legs." + m)


def test_bench_py_still_names_the_contract_fields():
    src = open(os.path.join(ROOT, "bench.py")).read()
    for key in ('"metric"', '"value"', '"unit"', '"n_gpus"', '"steps"', '"warmup"', '"ms_per_step"', '"higher_is_better"', '"scaling"',
                '"vs_baseline"', '"dtype"', '"data"', '"config"', '"roofline"', '"cpu_baseline"'):
        assert key in src, key


def test_dump_outputs_writes_the_returned_rows_exactly(tmp_path, monkeypatch):
    """bench.py --dump-outputs: only the keypoints a caller receives (counts per image), every field and descriptor bit exact
    in float32 / float64; past the size budget a fixed seeded sample of the rows, with their row numbers."""
    import numpy as np
    import torch
    import msorb
    import bench
    rng = np.random.default_rng(3)
    n, cap = 5, 64
    counts = np.array([64, 0, 7, 30, 1], np.int32)
    kp = np.zeros((n, cap), msorb.KP_DTYPE)
    for f in msorb.KP_DTYPE.names:
        kp[f] = rng.integers(-1, 2000, (n, cap)) if f in ("octave", "class_id") else rng.random((n, cap)) * 1241
    d_kps = torch.from_numpy(kp.view(np.uint8).reshape(n, cap, 28).copy())
    d_desc = torch.from_numpy(rng.integers(0, 256, (n, cap, 32), dtype=np.uint8))
    want_kp = np.concatenate([kp[i, :c] for i, c in enumerate(counts)])
    want_desc = np.concatenate([d_desc.numpy()[i, :c] for i, c in enumerate(counts)])
    bench.dump_outputs(str(tmp_path / "all"), counts, counts - 1, d_kps, d_desc)
    k, w = np.load(tmp_path / "all" / "keypoints.npy"), np.load(tmp_path / "all" / "descriptors.npy")
    assert np.load(tmp_path / "all" / "counts.npy").tolist() == counts.tolist()
    assert np.load(tmp_path / "all" / "mono.npy").tolist() == (counts - 1).tolist()
    assert k.dtype == np.float32 and w.dtype == np.float64 and len(k) == len(w) == counts.sum()
    for j, f in enumerate(msorb.KP_DTYPE.names):
        assert np.array_equal(k[:, j], want_kp[f].astype(np.float32)), f
    assert np.array_equal(w.astype(np.uint32).view(np.uint8).reshape(-1, 32), want_desc)
    assert not (tmp_path / "all" / "keypoint_index.npy").exists()
    monkeypatch.setattr(bench, "DUMP_BUDGET", 3000)
    for run in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / run), counts, counts, d_kps, d_desc)
    idx = np.load(tmp_path / "s1" / "keypoint_index.npy").astype(np.int64)
    assert 0 < len(idx) < counts.sum() and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "s1" / "keypoints.npy"), k[idx])
    assert np.array_equal(np.load(tmp_path / "s1" / "descriptors.npy"), w[idx])
    assert sum(a.nbytes for a in (np.load(tmp_path / "s1" / f) for f in ("counts.npy", "mono.npy", "keypoints.npy", "descriptors.npy",
                                                                           "keypoint_index.npy"))) <= 3000
    assert np.array_equal(np.load(tmp_path / "s2" / "keypoint_index.npy"), idx)
