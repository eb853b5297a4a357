"""The FAST kernel's last phase on the device against the CPU oracle: per-level candidate lists (x, y, score, in emission order), as
tests/test_extractor_gpu.py compares them, on scenes built to sit where that phase can go wrong (tests/fast_emission_scenes.py):

  words      kept corners on both sides of every bitmap word boundary of a row, in the first and the last word of a cell, six in one
             word (the per-lane emission loop) and in both words of one row
  spare      a stronger corner in the first row below every cell's detection area, right under a weaker one in its last row: a spare
             row that raised a flag would cost the weaker one.  Cells of both ways of dealing rows to threads (CellDesc::by_wave 0 and
             1) have such rows in the 128-thread geometry; in the 256-thread one only by_wave 0 occurs
  retry      cells with corners only between minThFAST and iniThFAST (planes cleared, second pass emits), cells that stay empty
  saturated  one cell with more quick-test survivors than the work list holds (its own scan and emission) beside ordinary cells

in three geometries — 122 x 259 (every cell small: fast_cells_kernel<., GeoSmall>, 128 threads, two words per row), 92 x 259 (one row
of cells 60 rows tall: GeoLarge, 256 threads) and 101 x 101 (one 69 x 69 cell: GeoLarge with the third word of a row in use) — and
through every launch that shares the body: a single frame, a small batch with padded rows (ALIGNED), the same batch tightly packed
(259 and 101 columns are not 4-byte aligned: the byte-granular variant), and MSORB_FRAME_FUSE=1 (frame_fast_blur_kernel).

Each case first asserts from the oracle's output that its scene does what it is meant to (fes.check)."""
import numpy as np
import pytest

import fast_emission_scenes as fes

pytestmark = pytest.mark.gpu


def _extractor(msorb_mod, s):
    return msorb_mod.ORBextractor(300, 1.2, s["geom"][2], fes.INI_TH, fes.MIN_TH)


def _assert_candidates(ex, s, image, what):
    for l in range(s["geom"][2]):
        got, want = ex.debug_candidates(image, l), s["cand"][l]
        assert got.shape == want.shape and np.array_equal(got, want), f"{what}: FAST candidates of image {image}, level {l}"


def _assert_features(kps, desc, s):
    _, rkps, rdesc = s["ref"]
    assert len(kps) == len(rkps)
    for f in ("octave", "x", "y", "response", "size", "angle", "class_id"):
        assert np.array_equal(kps[f].view(np.uint32), rkps[f].view(np.uint32)), f"keypoint field {f} differs"
    assert np.array_equal(desc, rdesc)


def _frame(msorb_mod, s, what):
    ex = _extractor(msorb_mod, s)
    try:
        mono, kps, desc = ex(s["img"])
        _assert_candidates(ex, s, 0, what)
        assert mono == s["ref"][0]
        _assert_features(kps, desc, s)
    finally:
        ex.close()


def _batch(msorb_mod, s, n, aligned, what):
    import torch
    rows, cols, _ = s["geom"]
    pitch = (cols + 63) // 64 * 64 if aligned else cols
    store = torch.zeros((n, rows, pitch), dtype=torch.uint8, device="cuda")
    view = store[:, :, :cols]
    view.copy_(torch.from_numpy(np.stack([s["img"]] * n)).cuda())
    assert (view.stride(1) % 4 == 0) == aligned
    ex = _extractor(msorb_mod, s)
    try:
        counts, mono, d_kps, d_desc = ex.extract_batch(view)
        for i in range(n):
            _assert_candidates(ex, s, i, what)
        kps = msorb_mod.keypoints_from_device(d_kps, counts)
        desc = d_desc.cpu().numpy()
        for i in range(n):
            assert mono[i] == s["ref"][0]
            _assert_features(kps[i], desc[i, :counts[i]], s)
    finally:
        ex.close()


@pytest.mark.parametrize("name", fes.NAMES)
def test_single_frame(msorb_mod, oracle, name):
    s = fes.scenes(msorb_mod, oracle)[name]
    fes.check(name, s)
    _frame(msorb_mod, s, "frame")


@pytest.mark.parametrize("name", fes.NAMES)
def test_batch_with_aligned_rows(msorb_mod, oracle, name):
    s = fes.scenes(msorb_mod, oracle)[name]
    fes.check(name, s)
    _batch(msorb_mod, s, 3, True, "aligned batch")


@pytest.mark.parametrize("name", fes.NAMES)
def test_batch_byte_granular(msorb_mod, oracle, name):
    """Tightly packed rows of 259 / 101 bytes stay in place in a small batch: fast_cells_kernel<false, .> evaluates the per-thread
    formulas (the rows a thread owns among them) instead of loading the table."""
    s = fes.scenes(msorb_mod, oracle)[name]
    fes.check(name, s)
    _batch(msorb_mod, s, 2, False, "byte-granular batch")


@pytest.mark.parametrize("name", fes.NAMES)
def test_frame_fused_launch(msorb_mod, oracle, monkeypatch, name):
    """MSORB_FRAME_FUSE=1 (read when the handle is created): FAST rides one launch with the blur, frame_fast_blur_kernel, for a
    frame and for a batch of two."""
    s = fes.scenes(msorb_mod, oracle)[name]
    fes.check(name, s)
    monkeypatch.setenv("MSORB_FRAME_FUSE", "1")
    _frame(msorb_mod, s, "fused frame")
    _batch(msorb_mod, s, 2, True, "fused pair")
