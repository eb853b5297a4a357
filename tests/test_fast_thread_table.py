"""The FAST kernel's per-thread table (ms-slam_amd/csrc/orb_host.h FastThreadRec, built on the host next to the cell table) against a
plain restatement of the formulas the kernel evaluated per thread before the table existed and still evaluates in its byte-granular
variant (orb_kernels.hip fast_cells_body): staging store offset, quick-test window offset, column mask, owned rows, work-list base.
Every cell of every geometry below, for 128- and 256-thread workgroups, every thread: nothing is sampled.  Needs no GPU."""
import numpy as np
import pytest

from msorb import synth

# the kernel's two workgroup shapes (orb_kernels.hip GeoSmall / GeoLarge): threads -> (tile pitch, staging lanes per tile row)
SHAPES = {128: (52, 16), 256: (84, 32)}

# the cameras of the benchmark and the tests, and the odd sizes tests/test_extractor_gpu.py runs (one-cell images, tight 751-pixel
# rows, 333 x 517, 240 x 320, and sizes in the range its random-geometry test draws from with 4 / 6 / 8 levels)
GEOMETRIES = {
    "kitti": synth.KITTI, "euroc": synth.EUROC, "euroc_yaml": synth.EUROC_YAML, "fourseasons": synth.FOURSEASONS,
    "small": dict(rows=240, cols=320, nfeatures=500, scale=1.2, nlevels=8),
    "odd": dict(rows=333, cols=517, nfeatures=700, scale=1.2, nlevels=8),
    "euroc_751": dict(rows=240, cols=751, nfeatures=1000, scale=1.2, nlevels=8),
    "cell_101x101": dict(rows=101, cols=101, nfeatures=300, scale=1.2, nlevels=1),
    "cell_101x171": dict(rows=101, cols=171, nfeatures=300, scale=1.2, nlevels=1),
    "cell_90x240": dict(rows=90, cols=240, nfeatures=300, scale=1.2, nlevels=1),
    "random_241x331_4": dict(rows=241, cols=331, nfeatures=500, scale=1.2, nlevels=4),
    "random_377x1099_6": dict(rows=377, cols=1099, nfeatures=1000, scale=1.2, nlevels=6),
    "random_479x653_8": dict(rows=479, cols=653, nfeatures=500, scale=1.2, nlevels=8),
}


def umul24(a, b):
    return ((a & 0xFFFFFF) * (b & 0xFFFFFF)) & 0xFFFFFFFF


def thread_record(cd, T, tid):
    """fast_cells_body's per-thread set-up for thread `tid` of a T-thread workgroup on cell `cd` (a dict of CellDesc fields)."""
    P, col_lanes = SHAPES[T]
    x0, rw, rh, G, magic = cd["x0"], cd["rw"], cd["rh"], cd["G"], cd["g_magic"]
    dh = rh - 6
    ga = x0 & ~3
    x_lo, x_hi = x0 + 3, x0 + rw - 3
    gx0 = x_lo & ~3
    c_lo = gx0 - ga
    lane, wave = tid & 63, tid >> 6
    # staging: lane column c = dword of the tile row, row r0 of the pass
    c, r0 = tid & (col_lanes - 1), tid // col_lanes
    lds_store = r0 * P + 4 * c
    # quick-test mapping
    if (cd["by_wave128"] if T == 128 else cd["by_wave256"]) == 0:
        strip = umul24(tid, magic) >> 20
        g_own = tid - strip * G
        R = cd["R128"] if T == 128 else cd["R256"]
        y_b = strip * R
    else:
        sw = wave * 8
        sl = umul24(lane, magic) >> 20
        g_own = lane - sl * G
        R = ((cd["rw128"] if T == 128 else cd["rw256"]) >> sw) & 255
        y_w = ((cd["yw128"] if T == 128 else cd["yw256"]) >> sw) & 255
        y_b = y_w + sl * R if sl < cd["spw"] else dh
    nrows = min(max(dh - y_b, 0), R)
    c_own = c_lo + 4 * g_own
    xg = ga + c_own
    vlo, vhi = min(max(x_lo - xg, 0), 4), min(max(x_hi - xg, 0), 4)
    hm = ((0x80808080 << (8 * vlo)) & 0xFFFFFFFF) & ((0x0080808080 >> (8 * (4 - vhi))) & 0xFFFFFFFF)
    if vlo >= 4:
        hm = 0
    tbase = (((y_b + 3) << 7) | c_own) & 0xFFFF
    colp = (umul24(y_b, P) + c_own) & 0xFFFFFFFF
    return lds_store, colp, hm, nrows | (tbase << 16)


@pytest.mark.parametrize("threads", sorted(SHAPES))
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_every_record_is_what_the_kernel_computed(msorb_mod, name, threads):
    g = GEOMETRIES[name]
    cells, recs, n_classes = msorb_mod.fast_thread_table(g["rows"], g["cols"], g["nfeatures"], g["scale"], g["nlevels"], threads)
    assert len(cells) > 0 and n_classes > 0 and len(recs) == n_classes * threads
    seen = set()
    for i, row in enumerate(cells):
        cd = {k: int(v) for k, v in zip(msorb_mod.FAST_CELL_FIELDS, row)}
        for k in ("g_magic", "rw128", "yw128", "rw256", "yw256", "tt_off"):   # unsigned fields of the int32 export
            cd[k] &= 0xFFFFFFFF
        off = cd["tt_off"]
        assert off % threads == 0 and off + threads <= len(recs), (name, i, off)
        seen.add(off)
        want = np.array([thread_record(cd, threads, t) for t in range(threads)], dtype=np.uint64).astype(np.uint32)
        got = recs[off:off + threads]
        bad = np.nonzero((want != got).any(axis=1))[0]
        assert len(bad) == 0, (name, threads, "cell", i, cd, "thread", int(bad[0]), want[bad[0]].tolist(), got[bad[0]].tolist())
    assert len(seen) == n_classes, "every class is some cell's, every cell has a class"


def test_kitti_table_is_small(msorb_mod):
    """The table has to live in every XCD's L2 beside the pyramid: classes, not cells, decide its size."""
    g = GEOMETRIES["kitti"]
    cells, recs, n_classes = msorb_mod.fast_thread_table(g["rows"], g["cols"], g["nfeatures"], g["scale"], g["nlevels"], 128)
    print(f"KITTI 1241x376, 128 threads: {len(cells)} cells, {n_classes} classes, {recs.nbytes} table bytes")
    assert n_classes < len(cells) and recs.nbytes <= 256 * 1024
