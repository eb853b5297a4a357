"""Scenes for the FAST kernel's last phase (orb_kernels.hip fast_cells_body: NMS into the keep bitmap, emission by the bitmap word's
owner, and the quick test's rows that a thread visits without owning them), and the arithmetic that says what a scene does to the kernel: which bitmap word a
kept corner falls into, which rows are a thread's spare rows, how many quick-test survivors a cell has.

Everything here runs on the CPU: the cell table comes from the host-only msorb.fast_thread_table, the corners from the oracle.
tests/test_fast_emission_scenes.py asserts the situations without a GPU, tests/test_fast_emission_gpu.py runs the scenes on the
device and asserts the same situations again from the oracle's output, so a scene that drifts fails instead of passing vacuously.

Building blocks: a single pixel of value v on a flat background b is a FAST corner of score |v - b| - 1 (its whole circle is darker),
and pixels two or more columns apart on one row, or in rows two apart, do not lie on each other's circles or in each other's 3 x 3 NMS
window.  Two kept corners can never sit in adjacent columns of one row (the NMS is strict), so "columns 31 and 32" are on rows four
apart, and one row carries kept corners in both of its bitmap words."""
import numpy as np

MIN_BORDER = 16              # candidate coordinates are relative to (16, 16): EDGE_THRESHOLD - 3
INI_TH, MIN_TH = 20, 7
BG = 100

# (rows, cols, levels).  SMALL: every cell ROI <= 46 x 57, the 128-thread shape (GeoSmall, two bitmap words per row); cells of
# both ways of dealing rows to threads (by_wave 0 and 1) with rows to spare.  LARGE: one row of cells 70 rows tall, the 256-thread
# shape (GeoLarge, three words per row); its cells are narrow (a cell wider than 64 columns is the only one of its level), so WIDE
# is one 69 x 69 cell whose rows reach into the third word.  259 or 101 columns tightly packed are rows that are not 4-byte aligned.
SMALL = (122, 259, 3)
LARGE = (92, 259, 2)
WIDE = (101, 101, 2)
KINDS = {"small": ("words", "spare", "retry", "saturated"), "large": ("spare", "retry"), "wide": ("words", "saturated")}
NAMES = [f"{tag}_{kind}" for tag, kinds in KINDS.items() for kind in kinds]
SHAPE = {128: dict(work_cap=1536, wpr=2, max_r=5), 256: dict(work_cap=4096, wpr=3, max_r=6)}


def cell_table(msorb_mod, geom, threads):
    rows, cols, nlev = geom
    cells, _, _ = msorb_mod.fast_thread_table(rows, cols, 300, 1.2, nlev, threads)
    out = []
    for row in cells:
        cd = {k: int(v) for k, v in zip(msorb_mod.FAST_CELL_FIELDS, row)}
        for k in ("g_magic", "rw128", "yw128", "rw256", "yw256", "tt_off"):
            cd[k] &= 0xFFFFFFFF
        cd["dh"], cd["x_lo"], cd["x_hi"] = cd["rh"] - 6, cd["x0"] + 3, cd["x0"] + cd["rw"] - 3
        cd["gx0"] = cd["x_lo"] & ~3          # level column of bit 0 of the cell's bitmap rows
        cd["y_lo"] = cd["y0"] + 3            # level row of detection row 0
        out.append(cd)
    return out


def threads_of(cells):
    """The workgroup shape the library picks for a geometry (extractor.hip small_cells)."""
    return 128 if all(c["rw"] <= 46 and c["rh"] <= 57 for c in cells) else 256


def thread_rows(cd, T):
    """Per thread of a T-thread workgroup: (column group, first detection row, rows owned, iterations of the row loop), as
    fast_cells_body deals them (tests/test_fast_thread_table.py checks the same formulas against the host's table)."""
    G, magic, dh = cd["G"], cd["g_magic"], cd["dh"]
    out = []
    for tid in range(T):
        lane, wave = tid & 63, tid >> 6
        if (cd["by_wave128"] if T == 128 else cd["by_wave256"]) == 0:
            strip = (tid * magic) >> 20
            g, R = tid - strip * G, cd["R128"] if T == 128 else cd["R256"]
            y_b = strip * R
        else:
            sl = (lane * magic) >> 20
            g = lane - sl * G
            R = ((cd["rw128"] if T == 128 else cd["rw256"]) >> (8 * wave)) & 255
            y_w = ((cd["yw128"] if T == 128 else cd["yw256"]) >> (8 * wave)) & 255
            y_b = y_w + sl * R if sl < cd["spw"] else dh
        out.append((g, y_b, min(max(dh - y_b, 0), R), R))
    return out


def spare_row_threads(cd, T):
    """Threads for which detection row dh — the first row below the cell's detection area — is one of the rows the quick test's
    row loop visits without the thread owning it: a flag raised there must be masked."""
    return [t for t, (g, y_b, nrows, R) in enumerate(thread_rows(cd, T)) if g < cd["G"] and y_b <= cd["dh"] < y_b + max(R, 3) and nrows < max(R, 3)]


def by_wave(cd, T):
    return cd["by_wave128"] if T == 128 else cd["by_wave256"]


def cell_of(cells, level, x, y):
    """The cell whose detection area holds level pixel (x, y)."""
    for cd in cells:
        if cd["level"] == level and cd["x_lo"] <= x < cd["x_hi"] and cd["y_lo"] <= y < cd["y_lo"] + cd["dh"]:
            return cd
    return None


def kept_in_cell(cand, cd):
    """Rows of an oracle candidate list (x, y, score; relative to MIN_BORDER) inside the cell -> (bx, by, score): column inside the
    cell's group span and detection row, the coordinates of the keep bitmap."""
    x, y = cand[:, 0] + MIN_BORDER, cand[:, 1] + MIN_BORDER
    m = (x >= cd["x_lo"]) & (x < cd["x_hi"]) & (y >= cd["y_lo"]) & (y < cd["y_lo"] + cd["dh"])
    return np.stack([x[m] - cd["gx0"], y[m] - cd["y_lo"], cand[m, 2]], 1)


def words_of(kept, wpr):
    return kept[:, 1] * wpr + (kept[:, 0] >> 5)


def quick_survivors(img, cd, th):
    """(pixel, polarity) pairs of the cell that pass the kernel's quick test at `th`: one of up / down AND one of left / right, three
    pixels away, darker than v - th (or brighter than v + th).  More than the shape's work_cap: the saturated-cell branch."""
    p = img.astype(np.int32)
    ys, xs = slice(cd["y_lo"], cd["y_lo"] + cd["dh"]), slice(cd["x_lo"], cd["x_hi"])
    sh = lambda dy, dx: p[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    v, U, D, L, R = sh(0, 0), sh(-3, 0), sh(3, 0), sh(0, -3), sh(0, 3)
    dark = ((U < v - th) | (D < v - th)) & ((L < v - th) | (R < v - th))
    bright = ((U > v + th) | (D > v + th)) & ((L > v + th) | (R > v + th))
    return int(dark.sum() + bright.sum())


def _flat(geom):
    return np.full(geom[:2], BG, np.uint8)


def _sprinkle(img, cells, skip=(), seed=1, value=(150, 256)):
    """A few isolated corners in every level-0 cell but `skip` (on a 6-pixel lattice, so none disturbs another)."""
    rng = np.random.default_rng(seed)
    for cd in cells:
        if cd["level"] != 0 or cd in skip:
            continue
        for _ in range(6):
            x = cd["x_lo"] + 6 * int(rng.integers(0, max(1, (cd["x_hi"] - cd["x_lo"] - 1) // 6)))
            y = cd["y_lo"] + 3 + 6 * int(rng.integers(0, max(1, (cd["dh"] - 7) // 6)))
            img[y, x] = int(rng.integers(*value))
    return img


def widest_cell(cells):
    return max((c for c in cells if c["level"] == 0), key=lambda c: (c["x_hi"] - c["gx0"], c["dh"]))


def scene_words(cells, geom, wpr):
    """Kept corners at the bitmap's word boundaries in the widest level-0 cell: columns 31 and 32 (rows four apart), 63 and 64 where
    the row has a third word; first and last word of the cell; six corners in one word and two in the next word of the same row."""
    img = _flat(geom)
    cd = widest_cell(cells)
    span = cd["x_hi"] - cd["gx0"]                      # bitmap columns in use: [x_lo - gx0, span)
    put = lambda bx, by, v: img.__setitem__((cd["y_lo"] + by, cd["gx0"] + bx), v)
    first = cd["x_lo"] - cd["gx0"]
    for i, bx in enumerate(range(first, 30, 4)):       # first word of the cell: detection row 0, from the first column on
        put(bx, 0, 250 - 7 * i)
    for i, bx in enumerate(range(span - 1, 32 * (wpr - 1) - 1, -4)):   # last word: last detection row, up to the last column
        put(bx, cd["dh"] - 1, 140 + 9 * i)
    for k in range(1, wpr):
        if 32 * k < span:
            put(32 * k - 1, 6, 220)
            put(32 * k, 10, 230)
    for i, bx in enumerate((20, 22, 24, 26, 28, 30, 32, 34)):  # one row, both words, six of them in the first
        put(bx, 16, 200 + 5 * i)
    return _sprinkle(img, cells, skip=(cd,), seed=2), cd


def check_words(cand0, cd, wpr):
    kept = kept_in_cell(cand0, cd)
    at = {(int(bx), int(by)) for bx, by, _ in kept}
    w = words_of(kept, wpr)
    span = cd["x_hi"] - cd["gx0"]
    assert span > 32 * (wpr - 1), "the cell's rows reach into their last bitmap word"
    for k in range(1, wpr):
        assert (32 * k - 1, 6) in at and (32 * k, 10) in at, f"kept corners at columns {32 * k - 1} and {32 * k}"
    assert 0 in w and cd["dh"] * wpr - 1 in w, "first and last word of the cell"
    assert (span - 1, cd["dh"] - 1) in at and (cd["x_lo"] - cd["gx0"], 0) in at, "first and last detection pixel of the cell"
    assert np.bincount(w).max() >= 6, "six kept corners in one word"
    assert {16 * wpr, 16 * wpr + 1} <= set(w.tolist()), "both words of one row"


def scene_spare(cells, geom):
    """Under every level-0 cell: a corner of score 99 in its last detection row and a stronger one (154) right below it, in the
    first row the cell does NOT detect in (the ROI's border: the cell below owns it, or nobody in the last row of cells).  A thread
    whose spare row raised a flag there would score the stronger one, and the NMS would drop the weaker: a missing candidate."""
    img = _flat(geom)
    for cd in cells:
        if cd["level"] != 0:
            continue
        y = cd["y_lo"] + cd["dh"]
        for x in range(cd["x_lo"], cd["x_hi"], 5):   # step 5: every pixel position of a 4-pixel group comes up
            img[y - 1, x] = 200
            img[y, x] = 255
    return img


def check_spare(cand0, cells, T, want_modes):
    """want_modes: the ways of dealing rows (CellDesc::by_wave) under which some cell of the scene has rows to spare"""
    modes = set()
    for cd in cells:
        if cd["level"] != 0:
            continue
        kept = kept_in_cell(cand0, cd)
        last = kept[kept[:, 1] == cd["dh"] - 1]
        want = list(range(cd["x_lo"] - cd["gx0"], cd["x_hi"] - cd["gx0"], 5))
        assert last[:, 0].tolist() == want and np.all(last[:, 2] == 99), "the weaker corners of the last row are the oracle's"
        if spare_row_threads(cd, T):
            modes.add(by_wave(cd, T))
    assert modes == want_modes, "cells with spare rows under these ways of dealing the rows"


def scene_retry(cells, geom):
    """Level-0 cells in turn: strong corners (first pass), only corners between minTh and iniTh (the retry finds them), nothing."""
    img = _flat(geom)
    kinds = {}
    for i, cd in enumerate(c for c in cells if c["level"] == 0):
        kinds[i] = i % 3
        if i % 3 == 2:
            continue
        for k, x in enumerate(range(cd["x_lo"], cd["x_hi"], 4)):
            y = cd["y_lo"] + (7 * k) % cd["dh"]
            img[y, x] = (BG + 60 + k) if i % 3 == 0 else (BG + MIN_TH + 1 + k % (INI_TH - MIN_TH - 1)) if k % 2 else (BG - MIN_TH - 1 - k % 5)
    return img, kinds


def check_retry(cand0, stats0, cells):
    total, retried, empty = stats0
    n0 = sum(1 for c in cells if c["level"] == 0)
    assert total == n0 and retried == n0 - (n0 + 2) // 3 and empty == n0 // 3, stats0
    weak = cand0[cand0[:, 2] < INI_TH]
    assert len(weak) > 10 and weak[:, 2].min() >= MIN_TH and len(cand0) - len(weak) > 10


def scene_saturated(cells, geom, T):
    """A diagonal ramp of 12 grey levels per pixel (wrapping) under a little noise over the whole ROI of the widest level-0 cell:
    three pixels away one of up / left is brighter by more than iniTh and one of down / right darker, so most pixels pass the quick
    test in BOTH polarities — uniform noise gives 0.9 survivors per pixel, too few to overflow the 256-thread shape's list on the
    largest cell there is.  The wraps and the noise make a few hundred of them corners.  Isolated corners everywhere else."""
    img = _flat(geom)
    cd = widest_cell(cells)
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:cd["rh"], 0:cd["rw"]]
    img[cd["y0"]:cd["y0"] + cd["rh"], cd["x0"]:cd["x0"] + cd["rw"]] = ((xx + yy) * 12 + rng.integers(0, 256, xx.shape) // 6) % 256
    return _sprinkle(img, cells, skip=(cd,), seed=6), cd


def check_saturated(img, cand0, cd, cells, T):
    assert quick_survivors(img, cd, INI_TH) > SHAPE[T]["work_cap"], "more quick-test survivors than the work list holds"
    assert len(kept_in_cell(cand0, cd)) > 50
    for c in cells:   # the common path beside it
        if c["level"] == 0 and c is not cd:
            assert 0 < quick_survivors(img, c, INI_TH) <= SHAPE[T]["work_cap"] and len(kept_in_cell(cand0, c)) > 0


_CACHE = {}


def scenes(msorb_mod, oracle):
    """name -> dict(geom, T, cells, img, focus, cand [per level], stats, ref (mono, keypoints, descriptors)): every scene with the
    oracle's answer, computed once per session and left unchanged; `check(name, s)` asserts the scene's situation from it."""
    if _CACHE:
        return _CACHE
    for tag, geom in (("small", SMALL), ("large", LARGE), ("wide", WIDE)):
        T = threads_of(cell_table(msorb_mod, geom, 128))
        cells = cell_table(msorb_mod, geom, T)
        assert T == (128 if tag == "small" else 256), "the geometry routes to the intended workgroup shape"
        make = {"words": lambda: scene_words(cells, geom, SHAPE[T]["wpr"]), "spare": lambda: (scene_spare(cells, geom), None),
                "retry": lambda: (scene_retry(cells, geom)[0], None), "saturated": lambda: scene_saturated(cells, geom, T)}
        for name in KINDS[tag]:
            img, focus = make[name]()
            ref = oracle.OracleExtractor(300, 1.2, geom[2], INI_TH, MIN_TH)
            out = ref(img)
            _CACHE[f"{tag}_{name}"] = dict(geom=geom, T=T, cells=cells, img=img, focus=focus, ref=out, stats=ref.cell_stats(),
                                           cand=[ref.candidates(l).copy() for l in range(geom[2])])
    return _CACHE


def check(name, s):
    (tag, kind), T, cand0 = name.split("_"), s["T"], s["cand"][0]
    if kind == "words":
        check_words(cand0, s["focus"], SHAPE[T]["wpr"])
    elif kind == "spare":
        # (the 256-thread shape deals rows per wave only for cells wider than this geometry's)
        check_spare(cand0, s["cells"], T, {0, 1} if tag == "small" else {0})
    elif kind == "retry":
        check_retry(cand0, s["stats"][0], s["cells"])
    else:
        check_saturated(s["img"], cand0, s["focus"], s["cells"], T)
