"""Every entry of the extractor under every switch that changes how its host side issues the stages: the one pipeline of
csrc/extractor.hip (pyramid, blur, FAST, compaction, selection, describe, counts) against the CPU oracle, bit for bit, at the
`small` configuration of test_extractor_gpu.py.

The switches are read when a handle is created, so every case makes its own handle under monkeypatch.setenv.  Where an entry
refuses to run in a mode (it needs the device pipeline) the case asserts the refusal: MSORB_E_INVALID and the text of
msorb_last_error.  The refusing handle has extracted one image before: `device_quadtree` follows MSORB_QUADTREE=host only once
the geometry is set, so a handle that has never seen an image does not refuse under that switch (a finding about the entry
checks, which read that flag before they set the geometry; not changed here)."""
import numpy as np
import pytest

from msorb import synth
import matcher_cases as mc

pytestmark = pytest.mark.gpu

CFG = dict(rows=240, cols=320, nfeatures=500, scale=1.2, nlevels=8, ini_th=20, min_th=7)
MBF, MB = mc.KITTI_BF, mc.KITTI_BF / mc.KITTI_FX

# name -> (environment at creation, calls on the fresh handle)
MODES = {
    "default": ({}, ()),
    "serial": ({"MSORB_SERIAL_PIPELINE": "1"}, ()),
    "host_quadtree": ({"MSORB_QUADTREE": "host", "MSORB_HOST_THREADS": "2"}, ()),
    "global_quadtree": ({"MSORB_QUADTREE": "global"}, ()),
    "profiling": ({}, (("set_profiling", (True,)),)),
    "one_group_blur_on_main": ({}, (("set_overlap", (1, False)),)),
    "frame_fuse_0": ({"MSORB_FRAME_FUSE": "0"}, ()),
    "frame_fuse_1": ({"MSORB_FRAME_FUSE": "1"}, ()),
    "frame_fuse_2": ({"MSORB_FRAME_FUSE": "2"}, ()),
    "frame_compact_0": ({"MSORB_FRAME_COMPACT": "0"}, ()),
}
NO_DEVICE_PIPELINE = ("serial", "host_quadtree")
REFUSES = {   # entry -> (modes that refuse, the text)
    "pair": (NO_DEVICE_PIPELINE + ("profiling",), "msorb_extract_pair needs the device pipeline"),
    "stereo": (NO_DEVICE_PIPELINE, "msorb_extract_stereo needs the device pipeline"),
    "split": (NO_DEVICE_PIPELINE, "msorb_extract_stereo_split needs the device pipeline"),
    "submit": (NO_DEVICE_PIPELINE, "msorb_extract_batch_submit needs the device pipeline"),
}


def _oracle(oracle):
    return oracle.OracleExtractor(CFG["nfeatures"], CFG["scale"], CFG["nlevels"], CFG["ini_th"], CFG["min_th"])


@pytest.fixture(scope="module")
def want(oracle):
    """The oracle's answers, computed once: 17 images (the batches; image 0 is the one-image call) and one stereo pair."""
    ref = _oracle(oracle)
    imgs = np.stack([synth.image(400 + i, CFG["rows"], CFG["cols"]) for i in range(17)])
    out = {"imgs": imgs, "single": [], "levels": None}
    for i in range(17):
        out["single"].append(ref(imgs[i]))
        if i == 0:
            out["levels"] = [ref.level(l).copy() for l in range(CFG["nlevels"])]
    L, R = synth.stereo_pair(77, CFG["rows"], CFG["cols"])
    orl, orr = _oracle(oracle), _oracle(oracle)
    out["L"], out["R"] = L, R
    out["eyes"] = [orl(L), orr(R)]
    out["eye_levels"] = [[o.level(l).copy() for l in range(CFG["nlevels"])] for o in (orl, orr)]
    tb = orl.tables()
    out["stereo"] = oracle.compute_stereo_matches(out["eyes"][0][1], out["eyes"][0][2], out["eyes"][1][1], out["eyes"][1][2],
                                                  out["eye_levels"][0], out["eye_levels"][1], tb["scale"], tb["inv_scale"], MB, MBF)
    return out


def _handle(msorb_mod, monkeypatch, mode):
    env, calls = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ex = msorb_mod.ORBextractor(CFG["nfeatures"], CFG["scale"], CFG["nlevels"], CFG["ini_th"], CFG["min_th"])
    for name, args in calls:
        getattr(ex, name)(*args)
    return ex


def _assert_same(kps, desc, rkps, rdesc):
    assert len(kps) == len(rkps)
    for f in ("octave", "x", "y", "response", "size", "angle", "class_id"):
        assert np.array_equal(kps[f].view(np.uint32), rkps[f].view(np.uint32)), f"keypoint field {f} differs"
    assert np.array_equal(desc, rdesc)


def _refused(msorb_mod, entry, mode, ex, want, call):
    """True when `entry` refuses in `mode`: then the refusal is asserted, on a handle whose geometry is set."""
    modes, text = REFUSES.get(entry, ((), ""))
    if mode not in modes:
        return False
    mono, kps, desc = ex(want["imgs"][0])
    _assert_same(kps, desc, want["single"][0][1], want["single"][0][2])
    with pytest.raises(msorb_mod.MsorbError) as e:
        call()
    assert e.value.code == msorb_mod.E_INVALID and text in str(e.value), str(e.value)
    mono, kps, desc = ex(want["imgs"][0])          # the handle is as usable as before
    _assert_same(kps, desc, want["single"][0][1], want["single"][0][2])
    return True


def _assert_stages(ex):
    ms = ex.stage_ms()
    assert set(ms) == {"pyramid", "fast", "compact", "blur", "select", "describe"}
    assert all(np.isfinite(v) and v >= 0 for v in ms.values()), ms


@pytest.mark.parametrize("host_pyramid", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_one_image(msorb_mod, want, monkeypatch, mode, host_pyramid):
    ex = _handle(msorb_mod, monkeypatch, mode)
    try:
        ex.set_host_pyramid(host_pyramid)
        for _ in range(2):                          # a cold and a warm handle
            mono, kps, desc = ex(want["imgs"][0])
            rmono, rkps, rdesc = want["single"][0]
            assert mono == rmono
            _assert_same(kps, desc, rkps, rdesc)
            for l in range(CFG["nlevels"]):
                assert np.array_equal(ex.pyramid_level(l), want["levels"][l]), f"host pyramid level {l}"
        if mode == "profiling":
            _assert_stages(ex)
    finally:
        ex.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_pair(msorb_mod, want, monkeypatch, mode):
    ex = _handle(msorb_mod, monkeypatch, mode)
    try:
        ex.set_host_pyramid(True)
        if _refused(msorb_mod, "pair", mode, ex, want, lambda: ex.extract_pair(want["L"], want["R"])):
            return
        got = ex.extract_pair(want["L"], want["R"])
        for which in (0, 1):
            mono, kps, desc = got[which]
            rmono, rkps, rdesc = want["eyes"][which]
            assert mono == rmono
            _assert_same(kps, desc, rkps, rdesc)
            for l in range(CFG["nlevels"]):
                assert np.array_equal(ex.pyramid_level_image(which, l), want["eye_levels"][which][l]), (which, l)
    finally:
        ex.close()


def _assert_stereo(got, want):
    kl, dl, kr, dr, ur, dp, oob = got
    _assert_same(kl, dl, want["eyes"][0][1], want["eyes"][0][2])
    _assert_same(kr, dr, want["eyes"][1][1], want["eyes"][1][2])
    rur, rdp, roob = want["stereo"]
    assert np.array_equal(ur.view(np.uint32), rur.view(np.uint32)) and np.array_equal(dp.view(np.uint32), rdp.view(np.uint32))
    assert oob == roob and (ur > 0).sum() > 20


@pytest.mark.parametrize("mode", list(MODES))
def test_stereo(msorb_mod, want, monkeypatch, mode):
    ex = _handle(msorb_mod, monkeypatch, mode)
    try:
        if _refused(msorb_mod, "stereo", mode, ex, want, lambda: ex.extract_stereo(want["L"], want["R"], MB, MBF)):
            return
        for _ in range(2):
            _assert_stereo(ex.extract_stereo(want["L"], want["R"], MB, MBF), want)
    finally:
        ex.close()


@pytest.mark.parametrize("mode", NO_DEVICE_PIPELINE)
def test_split_refuses(msorb_mod, want, monkeypatch, mode):
    exl, exr = _handle(msorb_mod, monkeypatch, mode), _handle(msorb_mod, monkeypatch, mode)
    try:
        assert _refused(msorb_mod, "split", mode, exl, want, lambda: exl.extract_stereo_split(exr, want["L"], want["R"], MB, MBF))
    finally:
        exl.close()
        exr.close()


def _assert_batch(msorb_mod, want, n, got):
    counts, mono, d_kps, d_desc = got
    kps = msorb_mod.keypoints_from_device(d_kps, counts)
    desc = d_desc.cpu().numpy()
    assert len(counts) == n
    for i in range(n):
        rmono, rkps, rdesc = want["single"][i]
        assert counts[i] == len(rkps) and mono[i] == rmono, i
        _assert_same(kps[i], desc[i, :counts[i]], rkps, rdesc)


@pytest.mark.parametrize("n", [3, 17])      # 17: two sub-batches of 8 and 9 images where the mode runs more than one
@pytest.mark.parametrize("mode", list(MODES))
def test_batch(msorb_mod, want, monkeypatch, mode, n):
    import torch
    ex = _handle(msorb_mod, monkeypatch, mode)
    try:
        d = torch.from_numpy(want["imgs"][:n]).cuda()
        for _ in range(2):
            _assert_batch(msorb_mod, want, n, ex.extract_batch(d))
        if mode == "profiling":
            _assert_stages(ex)
    finally:
        ex.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_submit_wait(msorb_mod, want, monkeypatch, mode):
    import torch
    ex = _handle(msorb_mod, monkeypatch, mode)
    try:
        d = torch.from_numpy(want["imgs"]).cuda()
        if _refused(msorb_mod, "submit", mode, ex, want, lambda: ex.extract_batch_submit(d)):
            return
        for _ in range(2):
            ex.extract_batch_submit(d)
            _assert_batch(msorb_mod, want, 17, ex.extract_batch_wait())
        if mode == "profiling":
            _assert_stages(ex)
    finally:
        ex.close()
