"""CPU-only tests that pin the oracle itself: known answers from the reference's own constants
(SURVEY.md §8 header table, computed from the reference's YAMLs and ORBextractor.cc), hand-checkable
primitive cases, the pattern table against the stored record of the reference text, the restated glibc
sinf/cosf against the installed glibc, and the committed golden fixtures.

PARITY UNPINNED: the reference has no tests or golden vectors and its OpenCV primitives cannot run here,
so these tests pin the oracle to the written spec, not to OpenCV output."""
import hashlib
import json
import math
import os
import subprocess

import numpy as np
import pytest

from msorb import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_scale_tables_and_quota_known_answers(oracle):
    ex = oracle.OracleExtractor(2000, 1.2, 8, 20, 7)
    t = ex.tables()
    # mvScaleFactor accumulated in float (ORBextractor.cc:416-422), values from SURVEY.md §8
    want = [1.0, 1.2000000477, 1.4400000572, 1.7280001640, 2.0736002922, 2.4883203506, 2.9859845638, 3.5831816196]
    assert np.array_equal(t["scale"], np.array(want, np.float32))
    assert t["per_level"].tolist() == [434, 362, 302, 251, 209, 175, 145, 122]
    assert t["umax"].tolist() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    assert oracle.OracleExtractor(1200, 1.2, 8, 20, 7).tables()["per_level"].tolist() == [261, 217, 181, 151, 126, 105, 87, 72]
    assert oracle.OracleExtractor(1000, 1.2, 8, 20, 7).tables()["per_level"].tolist() == [217, 181, 151, 126, 105, 87, 73, 60]


@pytest.mark.parametrize("rows,cols,sizes", [
    (376, 1241, [(1241, 376), (1034, 313), (862, 261), (718, 218), (598, 181), (499, 151), (416, 126), (346, 105)]),
    (480, 752, [(752, 480), (627, 400), (522, 333), (435, 278), (363, 231), (302, 193), (252, 161), (210, 134)]),
    (400, 800, [(800, 400), (667, 333), (556, 278), (463, 231), (386, 193), (322, 161), (268, 134), (223, 112)]),
])
def test_level_sizes_known_answers(oracle, rows, cols, sizes):
    ex = oracle.OracleExtractor(500, 1.2, 8, 20, 7)
    ex(synth.image(0, rows, cols))
    assert [ex.level(l).shape[::-1] for l in range(8)] == sizes


def test_pattern_table_matches_reference_text():
    """orb_pattern.inc against the record of the reference's bit_pattern_31_ text in tests/golden/reference_constants.json
    (tools/make_reference_constants.py: digest, sums and end pairs of the 1024 numbers as the reference writes them)."""
    fix = json.load(open(os.path.join(GOLDEN, "reference_constants.json")))
    inc = open(os.path.join(ROOT, "ms-slam_amd", "csrc", "orb_pattern.inc")).read()
    mine = [int(v) for v in "".join(l for l in inc.splitlines() if not l.startswith("//")).replace(",", " ").split()]
    assert len(mine) == 1024 and all(-13 <= v <= 13 for v in mine)
    assert hashlib.sha256(np.array(mine, np.int8).tobytes()).hexdigest() == fix["pattern_sha256"]
    assert mine[:4] == fix["pattern_first_pair"] and mine[-4:] == fix["pattern_last_pair"]
    assert sum(mine) == fix["pattern_sum"] and sum(abs(v) for v in mine) == fix["pattern_abs_sum"]


def test_resize_constant_and_ramp(oracle):
    const = np.full((50, 60), 77, np.uint8)
    assert np.all(oracle.resize_linear_u8(const, 42, 50) == 77)
    # hand-computed tap: dst x=0 of a 6->5 resize: fx=(0.5*1.2-0.5)=0.1 -> weights 1843/205, src (10,20)
    src = np.tile(np.array([10, 20, 30, 40, 50, 60], np.uint8), (6, 1))
    out = oracle.resize_linear_u8(src, 5, 5)
    h = 10 * 1843 + 20 * 205
    b0, b1 = 1843, 205
    assert out[0, 0] == ((((b0 * (h >> 4)) >> 16) + ((b1 * (h >> 4)) >> 16) + 2) >> 2)
    # dst x=4: fx=4.9 -> src (50,60) weights 205/1843 -> 120830/2048 = 59
    assert out[0, 4] == 59 and out[0].tolist() == out[4].tolist()


def test_gaussian_constant_impulse_and_border(oracle):
    assert np.all(oracle.gaussian7(np.full((20, 30), 200, np.uint8)) == 200)
    imp = np.zeros((21, 21), np.uint8)
    imp[10, 10] = 255
    out = oracle.gaussian7(imp).astype(int)
    k = np.array([18, 34, 48, 56, 48, 34, 18])
    want = (np.outer(k, k) * 255 + 32768) >> 16
    assert np.array_equal(out[7:14, 7:14], want)
    # reflect-101 (gfedcb|abcdefgh): column -1 mirrors column 1, column 0 is not repeated
    edge = np.zeros((21, 21), np.uint8)
    edge[10, 0] = 255
    oe = oracle.gaussian7(edge).astype(int)
    assert oe[10, 0] == (56 * 56 * 255 + 32768) >> 16
    assert oe[10, 1] == (48 * 56 * 255 + 32768) >> 16
    edge1 = np.zeros((21, 21), np.uint8)
    edge1[10, 1] = 255
    assert oracle.gaussian7(edge1).astype(int)[10, 0] == ((48 + 48) * 56 * 255 + 32768) >> 16


def test_fast_known_corner(oracle):
    img = np.full((15, 15), 100, np.uint8)
    img[7, 7] = 200                      # isolated bright pixel: all 16 circle pixels darker by 100
    pts = oracle.fast9_nms(img, 20)
    assert pts.tolist() == [[7, 7, 99]]  # score = largest t with the test still firing = 100 - 1
    assert oracle.fast9_nms(img, 100).tolist() == []      # strict: needs p < v - t
    assert oracle.fast9_nms(img, 99).tolist() == [[7, 7, 99]]
    # an 8-pixel arc is not a corner, a 9-pixel arc is
    circ = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
            (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
    for n, expect in ((8, 0), (9, 1)):
        im = np.full((15, 15), 100, np.uint8)
        for dx, dy in circ[:n]:
            im[7 + dy, 7 + dx] = 160
        got = [p for p in oracle.fast9_nms(im, 20).tolist() if p[:2] == [7, 7]]
        assert len(got) == expect
    # NMS ties: two adjacent equal scores suppress each other (strict >)
    tie = np.full((15, 16), 100, np.uint8)
    tie[7, 7] = tie[7, 8] = 200
    assert all(p[:2] not in ([7, 7], [8, 7]) for p in oracle.fast9_nms(tie, 20).tolist())


def test_fast_atan2_against_atan2(oracle):
    rng = np.random.Generator(np.random.PCG64(1))
    for _ in range(2000):
        y, x = rng.integers(-200000, 200000, 2)
        if x == 0 and y == 0:
            continue
        want = math.degrees(math.atan2(y, x)) % 360
        got = oracle.fast_atan2(y, x)
        assert min(abs(got - want), 360 - abs(got - want)) < 0.35   # the polynomial's error is part of the result
    assert oracle.fast_atan2(0, 0) == 0 and oracle.fast_atan2(0, 5) == 0 and oracle.fast_atan2(5, 0) == 90
    assert oracle.fast_atan2(0, -5) == 180 and oracle.fast_atan2(-5, 0) == 270


def test_restated_glibc_sincosf_matches_installed_glibc(tmp_path):
    exe = tmp_path / "sincosf_check"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-mfma", "-o", str(exe),
                           os.path.join(ROOT, "tests", "sincosf_check.cc"), "-lm"])
    stride = "1" if os.environ.get("MSORB_EXHAUSTIVE") else "61"
    out = subprocess.check_output([str(exe), "0", "6.2831860", stride]).decode()
    assert "bad_plain=0 bad_fused=0" in out, out
    out = subprocess.check_output([str(exe), "6.2831860", "119.9", stride]).decode()
    assert "bad_fused=0" in out, out   # glibc's FMA ifunc variant is the one installed on FMA hosts


def test_operator_output_contract(oracle):
    cfg = synth.KITTI
    img = synth.image(21, cfg["rows"], cfg["cols"])
    ex = oracle.OracleExtractor(2000, 1.2, 8, 20, 7)
    mono, kps, desc = ex(img)
    assert mono == len(kps) and 1800 < len(kps) <= 2000 + 2 * 8     # ORBextractor.cc:746-747 overshoot bound
    assert np.all(np.diff(kps["octave"]) >= 0)                        # level-major when vLappingArea = {0,0}
    assert np.all(kps["size"] == np.floor(31 * ex.tables()["scale"][kps["octave"]]))
    assert np.all((kps["angle"] >= 0) & (kps["angle"] <= 360)) and np.all(kps["class_id"] == -1)
    lvl_x = kps["x"] / ex.tables()["scale"][kps["octave"]]
    assert lvl_x.min() >= 18.9                                        # EDGE_THRESHOLD
    mono2, kps2, desc2 = ex(img, (0, 1000))                           # mono call site Frame.cc:311
    assert mono2 < len(kps2) and sorted(map(bytes, desc2)) == sorted(map(bytes, desc))
    assert ex(np.zeros((0, 0), np.uint8))[0] == -1


def _digest(mono, kps, desc):
    h = hashlib.sha256()
    h.update(np.int32(mono).tobytes())
    h.update(np.ascontiguousarray(kps).view(np.uint8).tobytes())
    h.update(np.ascontiguousarray(desc).tobytes())
    return h.hexdigest()


def test_oracle_matches_committed_golden_fixtures(oracle):
    """tests/golden/extractor_golden.json was produced by tools/make_golden.py from this oracle (semantics
    version recorded inside); it guards against silent drift of the oracle and is what the GPU tests on the
    GPU box compare with when /root/reference is absent (it always is there)."""
    spec = json.load(open(os.path.join(GOLDEN, "extractor_golden.json")))
    assert spec["gauss_kernel_q88"] == [18, 34, 48, 56, 48, 34, 18]
    for case in spec["cases"]:
        img = synth.image(case["seed"], case["rows"], case["cols"])
        assert hashlib.sha256(img.tobytes()).hexdigest() == case["image_sha256"], "synthetic generator drifted"
        ex = oracle.OracleExtractor(case["nfeatures"], 1.2, 8, 20, 7)
        mono, kps, desc = ex(img, tuple(case["lapping"]))
        assert len(kps) == case["n_keypoints"] and mono == case["mono_index"]
        assert _digest(mono, kps, desc) == case["digest"]
        first = np.load(os.path.join(GOLDEN, case["head_file"]))
        assert np.array_equal(first["desc"], desc[:16]) and np.array_equal(first["kps"], kps[:16].view(np.uint8).reshape(16, 28))


# ---- second, independently structured numpy formulations of the three OpenCV primitives -------------------------
# (same published semantics as SURVEY.md Appendix A, written from the definitions rather than from the oracle's loops:
# they cannot pin the oracle to real OpenCV, but they do rule out slips inside the oracle's own restatement)

def _np_resize_linear(src, drows, dcols):
    def taps(dn, sn):
        scale = 1.0 / (float(dn) / sn)
        f = ((np.arange(dn) + 0.5) * scale - 0.5).astype(np.float32)
        i = np.floor(f).astype(np.int64)
        f = (f - i).astype(np.float32)
        f[i < 0] = 0
        i[i < 0] = 0
        hi = i >= sn - 1
        f[hi] = 0
        i[hi] = sn - 1
        a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)    # saturate_cast<short>(cvRound)
        a1 = np.rint(f * np.float32(2048)).astype(np.int64)
        return i, np.minimum(i + 1, sn - 1), a0, a1
    x0, x1, ca0, ca1 = taps(dcols, src.shape[1])
    y0, y1, cb0, cb1 = taps(drows, src.shape[0])
    s = src.astype(np.int64)
    H = s[:, x0] * ca0 + s[:, x1] * ca1
    return ((((cb0[:, None] * (H[y0] >> 4)) >> 16) + ((cb1[:, None] * (H[y1] >> 4)) >> 16) + 2) >> 2).astype(np.uint8)


def _np_gaussian7(src):
    k = np.array([18, 34, 48, 56, 48, 34, 18], np.int64)

    def refl(n):
        p = np.arange(-3, n + 3)
        p = np.where(p < 0, -p, p)
        return np.where(p >= n, 2 * (n - 1) - p, p)
    s = src.astype(np.int64)
    h = sum(k[t] * s[:, refl(src.shape[1])[t:t + src.shape[1]]] for t in range(7))
    v = sum(k[t] * h[refl(src.shape[0])[t:t + src.shape[0]], :] for t in range(7))
    return ((v + 32768) >> 16).astype(np.uint8)


def _np_fast_nms(img, th):
    """FAST-9/16 from the definition: corner(t) = some 9 contiguous circle pixels all > p+t or all < p-t; the score is
    the largest t for which the pixel is still a corner; keep strict 3x3 maxima; rows 3..h-4, cols 3..w-4."""
    circ = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1),
            (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
    h, w = img.shape
    s = img.astype(np.int64)
    c = s[3:h - 3, 3:w - 3]
    ring = np.stack([s[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in circ])      # [16, h-6, w-6]
    score = np.zeros_like(c)
    for sign in (1, -1):
        d = sign * (ring - c[None])                                                     # > t  <=> brighter / darker by t
        d2 = np.concatenate([d, d[:8]])
        arc_min = np.stack([d2[i:i + 9].min(0) for i in range(16)])                     # min over each 9-arc
        score = np.maximum(score, arc_min.max(0) - 1)                                   # largest t with min > t
    is_corner = score >= th                                                             # corner at th <=> max t >= th
    sc = np.where(is_corner, score, 0)
    pad = np.pad(sc, 1)
    nb = np.stack([pad[1 + dy:1 + dy + sc.shape[0], 1 + dx:1 + dx + sc.shape[1]]
                   for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)])
    keep = is_corner & (sc > nb.max(0))
    ys, xs = np.nonzero(keep)
    return np.stack([xs + 3, ys + 3, sc[ys, xs]], 1)


def test_oracle_primitives_against_definition_level_numpy(oracle):
    rng = np.random.default_rng(5)
    img = synth.image(11, 120, 173)
    noisy = np.clip(img.astype(np.int64) + rng.integers(-40, 41, img.shape), 0, 255).astype(np.uint8)
    for im in (img, noisy):
        for dr, dc in ((100, 144), (83, 120), (119, 172)):
            assert np.array_equal(oracle.resize_linear_u8(im, dr, dc), _np_resize_linear(im, dr, dc)), (dr, dc)
        assert np.array_equal(oracle.gaussian7(im), _np_gaussian7(im))
        for th in (7, 20, 60):
            got = oracle.fast9_nms(im, th)
            want = _np_fast_nms(im, th)
            order = np.lexsort((got[:, 0], got[:, 1])) if len(got) else []
            assert np.array_equal(got[order] if len(got) else got, want), th
    assert len(oracle.fast9_nms(noisy, 20)) > 50
