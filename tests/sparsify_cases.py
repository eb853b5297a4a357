"""Synthetic MapSparsification windows: 30 keyframes x ~1000 tracked points, 64x48 grid,
observation counts ~Geometric(mean 8), ~100 keyframes outside the window."""
import numpy as np


def window(seed, n_window=30, n_outside=100, n_points=6000, slots_per_kf=2000, tracked_frac=0.5, grid=(64, 48)):
    rng = np.random.Generator(np.random.PCG64(seed))
    n_kf = n_window + n_outside
    window_ids = np.sort(rng.choice(n_kf, n_window, replace=False))
    in_window = np.zeros(n_kf, np.uint8)
    in_window[window_ids] = 1
    bad = rng.random(n_points) < 0.05
    obs_lists = [set() for _ in range(n_points)]
    kf_slot_begin, slot_point, slot_cell = [0], [], []
    for k in window_ids:
        cells = np.sort(rng.integers(0, grid[0] * grid[1], slots_per_kf))   # grid walk order: col-major cell id
        tracked = rng.random(slots_per_kf) < tracked_frac
        pts = rng.choice(n_points, slots_per_kf, replace=False)
        for c, t, p in zip(cells, tracked, pts):
            if t:
                obs_lists[p].add(int(k))
                slot_point.append(-1 if bad[p] else int(p))
            else:
                slot_point.append(-1)
            slot_cell.append(int(c))
        kf_slot_begin.append(len(slot_point))
    outside = np.nonzero(in_window == 0)[0]
    for p in range(n_points):
        extra = min(rng.geometric(1 / 8.0) - 1, len(outside))
        if extra > 0:
            obs_lists[p].update(int(x) for x in rng.choice(outside, extra, replace=False))
    obs_begin, obs_kf = [0], []
    for p in range(n_points):
        obs_kf.extend(sorted(obs_lists[p]))
        obs_begin.append(len(obs_kf))
    point_nobs = np.diff(obs_begin).astype(np.int32)
    kf_num_mps = rng.integers(200, 1500, n_kf).astype(np.int32)
    return dict(kf_slot_begin=np.array(kf_slot_begin, np.int32), slot_point=np.array(slot_point, np.int32),
                slot_cell=np.array(slot_cell, np.int32), point_nobs=point_nobs, obs_begin=np.array(obs_begin, np.int32),
                obs_kf=np.array(obs_kf, np.int32), kf_in_window=in_window, kf_num_mps=kf_num_mps)


# ------------------------------------------------------------------------------------------------
# A plain reference of the matrix assembly, independent of oracle/sparsify_oracle.cc
# ------------------------------------------------------------------------------------------------
def reference_csr(w, N, n_max_obs_floor=0):
    """MapSparsification::Sparsifying up to model.setObjective (MapSparsification.cc:58-151), restated line by line on the flat
    arrays of a window: GRBLinExpr is a Python list of column indices (duplicate terms stay, as `+=` keeps them), the two
    std::map of :125-126 are one dict walked in ascending KeyFrame id.  Same dict as msorb.visibility_csr."""
    ksb = [int(x) for x in w["kf_slot_begin"]]
    sp, cell_of = w["slot_point"].tolist(), w["slot_cell"].tolist()
    nobs, ob, okf = w["point_nobs"].tolist(), w["obs_begin"].tolist(), w["obs_kf"].tolist()
    in_window, num_mps = w["kf_in_window"].tolist(), w["kf_num_mps"].tolist()
    K = len(ksb) - 1
    n_max = n_max_obs_floor                                   # :66-76 (the floor: map points of a KeyFrame outside its grid)
    for s in range(ksb[K]):
        if sp[s] >= 0 and nobs[sp[s]] > n_max:
            n_max = nobs[sp[s]]
    index = {}                                                # mnIndexForSparsification of the points marked with mnId
    local = []                                                # vLocalMapPoints
    rows = []                                                 # (kind, owner, rhs, terms) in addConstr order
    for k in range(K):                                        # :78-123
        expr_cons = []
        s, e = ksb[k], ksb[k + 1]
        while s < e:                                          # one grid cell = one run of equal slot_cell
            t = s
            while t < e and cell_of[t] == cell_of[s]:
                t += 1
            expr_cons_grid = []
            for i in range(s, t):                             # :88-110
                p = sp[i]
                if p < 0:
                    continue
                if p not in index:
                    index[p] = len(local)
                    local.append(p)
                expr_cons.append(index[p])
                expr_cons_grid.append(index[p])
            if expr_cons_grid:                                # bValidCell
                rows.append((0, cell_of[s], np.float32(1), expr_cons_grid))
            s = t
        rows.append((1, k, np.float32(N), expr_cons))
    extra = {}                                                # extraNum is len(), extraConstrints the list
    for c, p in enumerate(local):                             # :127-142
        for o in range(ob[p], ob[p + 1]):
            if not in_window[okf[o]]:
                extra.setdefault(okf[o], []).append(c)
    with np.errstate(divide="ignore", invalid="ignore"):
        for kf in sorted(extra):                              # :144-151, float arithmetic step by step
            n_mini = np.float32(len(extra[kf])) / np.float32(num_mps[kf]) * np.float32(N)
            rows.append((2, kf, n_mini, extra[kf]))
    row_begin = np.zeros(len(rows) + 1, np.int32)
    row_begin[1:] = np.cumsum([len(r[3]) for r in rows], dtype=np.int64)
    i32 = lambda v: np.array(v, np.int32).reshape(-1)
    return dict(n_cols=len(local), col_point=i32(local), obj_coef=np.array([n_max - nobs[p] for p in local], np.float32),
                n_rows=len(rows), row_begin=row_begin, row_kind=i32([r[0] for r in rows]), row_owner=i32([r[1] for r in rows]),
                row_rhs=np.array([r[2] for r in rows], np.float32), col_idx=i32([c for r in rows for c in r[3]]), n_max_obs=int(n_max))


CSR_SCALARS = ("n_cols", "n_rows", "n_max_obs")
CSR_ARRAYS = ("col_point", "obj_coef", "row_begin", "row_kind", "row_owner", "row_rhs", "col_idx")


def csr_differences(a, b):
    """Names of the fields in which two results differ; arrays by dtype, shape and BYTES (a NaN or the sign of a zero counts)."""
    bad = [k for k in CSR_SCALARS if int(a[k]) != int(b[k])]
    return bad + [k for k in CSR_ARRAYS
                  if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]


# ------------------------------------------------------------------------------------------------
# Structural windows: each one reaches a loop or an arm of csrc/visibility.hip that window() does not.  The sizes are the smallest
# that do, derived from these constants of the kernels; if one of them moves, the cases below have to be derived again
# (test_sparsify.py::test_case_constants_match_the_kernels reads them back from the source).
# ------------------------------------------------------------------------------------------------
LDS_HIST = 8192        # kLdsHist: vis_extra_count_body counts in LDS up to this many KeyFrames, with global atomics above
SCAN_CHUNK = 1024      # vis_extra_scan_kernel: KeyFrames per trip of its one workgroup, carry_r / carry_n between trips
COLUMNS_BLOCK = 256    # vis_flag_count_kernel / vis_columns_kernel: slots per block AND the stride of the block-count sum
INIT_GRID = 2048       # vis_init_kernel: grid cap, times COLUMNS_BLOCK threads = 524 288 words before the stride loop repeats
KF_THREADS = 1024      # kKfThreads: threads of the workgroup that walks one window KeyFrame

DEFAULT_N = 100


def split(w):
    """(arrays of the window, N, n_max_obs_floor): a case may carry its own "N" and "n_max_obs_floor"."""
    arrays = {k: v for k, v in w.items() if k not in ("N", "n_max_obs_floor")}
    return arrays, w.get("N", DEFAULT_N), w.get("n_max_obs_floor", 0)


def _assemble(kfs, n_points, obs_point, obs_kf, in_window, kf_num_mps, point_nobs=None, window_obs=True, **extra):
    """kfs: per window KeyFrame (slot_point, slot_cell).  (obs_point, obs_kf): observation pairs from outside; the pairs of the
    window's own valid slots are added, and every pair is kept once: a point's list holds a KeyFrame at most once."""
    in_window = np.asarray(in_window, np.uint8)
    n_kf = len(in_window)
    ids = np.nonzero(in_window)[0]
    assert len(ids) == len(kfs)
    pts = [np.asarray(p, np.int64).reshape(-1) for p, _ in kfs]
    cells = [np.asarray(c, np.int64).reshape(-1) for _, c in kfs]
    op, ok = [np.asarray(obs_point, np.int64).reshape(-1)], [np.asarray(obs_kf, np.int64).reshape(-1)]
    if window_obs:
        for k, p in enumerate(pts):
            op.append(p[p >= 0])
            ok.append(np.full((p >= 0).sum(), ids[k], np.int64))
    op, ok = np.concatenate(op), np.concatenate(ok)
    assert op.size == 0 or (0 <= op.min() and op.max() < n_points and 0 <= ok.min() and ok.max() < n_kf)
    key = np.unique(op * max(n_kf, 1) + ok)                      # sorted by point, then KeyFrame; no pair twice
    obs_begin = np.zeros(n_points + 1, np.int64)
    obs_begin[1:] = np.cumsum(np.bincount(key // max(n_kf, 1), minlength=n_points))
    slot_point = np.concatenate(pts + [np.zeros(0, np.int64)])
    assert slot_point.size == 0 or (-1 <= slot_point.min() and slot_point.max() < n_points)
    w = dict(kf_slot_begin=np.cumsum([0] + [len(p) for p in pts]).astype(np.int32), slot_point=slot_point.astype(np.int32),
             slot_cell=np.concatenate(cells + [np.zeros(0, np.int64)]).astype(np.int32),
             point_nobs=np.diff(obs_begin).astype(np.int32) if point_nobs is None else np.asarray(point_nobs, np.int32),
             obs_begin=obs_begin.astype(np.int32), obs_kf=(key % max(n_kf, 1)).astype(np.int32), kf_in_window=in_window,
             kf_num_mps=np.asarray(kf_num_mps, np.int32))
    w.update(extra)
    return w


def _random_kf(rng, n_slots, n_points, n_cells=64 * 48, valid=0.8, replace=False):
    cells = np.sort(rng.integers(0, n_cells, n_slots))
    pts = rng.choice(n_points, n_slots, replace=replace)
    pts[rng.random(n_slots) >= valid] = -1
    return pts, cells


def _random_outside(rng, n_points, outside, mean=4.0):
    cnt = np.minimum(rng.geometric(1.0 / mean, n_points) - 1, len(outside))
    return np.repeat(np.arange(n_points), cnt), outside[rng.integers(0, len(outside), cnt.sum())]


def _in_window(n_kf, ids):
    m = np.zeros(n_kf, np.uint8)
    m[list(ids)] = 1
    return m


def scan_carry(n_kf):
    """vis_extra_scan_kernel scans the KeyFrames in trips of SCAN_CHUNK = 1024 and carries the row rank and the non-zero offset
    from trip to trip.  n_kf = 1023 / 1024 end inside / exactly at the first trip, 1025 puts one KeyFrame into a second, 2049 one
    into a third.  Two window KeyFrames, about 270 columns; outside KeyFrames with a count lie in every trip, on both sides of
    every multiple of 1024 (indices 1023 | 1024, 2047 | 2048), and many have none, so rank and index differ."""
    rng = np.random.Generator(np.random.PCG64(1000 + n_kf))
    n_points, p = 300, np.arange(300)
    kfs = [_random_kf(rng, 200, n_points, 40, 0.9) for _ in range(2)]
    op, ok = [p, p, p[p % 2 == 0], p[p % 7 == 0]], [(p * 7 + 1) % n_kf, (p * 131 + 17) % n_kf, np.full(150, n_kf - 1), np.zeros(43, int)]
    for i, edge in enumerate(range(SCAN_CHUNK, n_kf + 1, SCAN_CHUNK)):
        for j, kf in enumerate((edge - 2, edge - 1, edge, edge + 1)):
            if kf < n_kf:
                sel = p[p % (2 + i + j) == 0]
                op.append(sel)
                ok.append(np.full(len(sel), kf))
    return _assemble(kfs, n_points, np.concatenate(op), np.concatenate(ok), _in_window(n_kf, (3, 600)),
                     rng.integers(200, 1500, n_kf))


def many_slots():
    """vis_columns_kernel sums the counts of the blocks in front of it with `for (i = tid; i < blockIdx.x; i += 256)`: the second
    trip of that loop needs blockIdx.x > 256, i.e. slot 257 * 256 = 65 792 and later.  33 KeyFrames of 2003 slots (two slots per
    thread of the KeyFrame workgroup, the last ones one) = 66 099 slots = blocks 0..258; 40 000 points keep first encounters
    coming up to the last block, block 256 (the first count of a second trip) included."""
    rng = np.random.Generator(np.random.PCG64(2001))
    n_points, n_kf = 40000, 33 + 50
    ids = np.sort(rng.choice(n_kf, 33, replace=False))
    kfs = [_random_kf(rng, 2003, n_points, valid=0.8) for _ in range(33)]
    m = _in_window(n_kf, ids)
    op, ok = _random_outside(rng, n_points, np.nonzero(m == 0)[0], 3.0)
    return _assemble(kfs, n_points, op, ok, m, rng.integers(200, 1500, n_kf))


def lds_hist_edge(n_kf):
    """vis_extra_count_body keeps one LDS counter per KeyFrame while n_kf_total <= kLdsHist = 8192 (n_kf * 4 bytes of dynamic LDS on
    top of the kernel's static 72) and turns to global atomics above: 8192 is the LDS arm at its limit, 8193 the other arm.
    Three window KeyFrames, about 1800 columns of about 2150 valid slots (67 and 69 bitmap words a row); the observations reach
    KeyFrames 0, 8191 and the last id.  With about 8190 outside KeyFrames the bitmap also passes the 524 288 words of init_stride()."""
    rng = np.random.Generator(np.random.PCG64(3000 + n_kf))
    n_points = 6000
    p = np.arange(n_points)
    kfs = [_random_kf(rng, 800, n_points, 600, 0.9) for _ in range(3)]
    sel = [p, p, p[p % 2 == 0], p[p % 3 == 0], p[p % 5 == 0], p[p % 11 == 0]]
    kf = [(p * 37 + 5) % n_kf, (p * 1009 + 77) % n_kf, n_kf - 1, n_kf - 2, LDS_HIST - 1, 0]
    ok = [np.broadcast_to(k, q.shape) for q, k in zip(sel, kf)]
    return _assemble(kfs, n_points, np.concatenate(sel), np.concatenate(ok), _in_window(n_kf, (10, 4000, 8000)),
                     rng.integers(200, 1500, n_kf))


def init_stride(shift=0):
    """vis_init_kernel clears the bitmaps with at most INIT_GRID = 2048 blocks of 256 threads and strides: words from 524 288 on
    are cleared by the second trip of `for (i = i0; i < bitmap_words; i += stride)`.  The bitmap has one row of ceil(cols_max / 32)
    words per KeyFrame outside the window (cols_max = valid slots, at most the points: 20 000 here): 9 window KeyFrames x 1900 slots give 15 289 valid slots =
    478 words, 1200 outside KeyFrames 573 600 words.  Every outside KeyFrame observes a few points, so the rows ranked 1097 and
    later, whose bits live beyond word 524 288, are in use.  Only a call that finds those words dirty can tell: init_stride(5)
    has the same slots and as many observations, so the same scratch layout, and sets other bits; it runs first, on the same thread."""
    rng = np.random.Generator(np.random.PCG64(4001))
    n_points, n_out = 20000, 1200
    n_kf = 9 + n_out
    ids = np.sort(rng.choice(n_kf, 9, replace=False))
    kfs = [_random_kf(rng, 1900, n_points, valid=0.9) for _ in range(9)]
    m = _in_window(n_kf, ids)
    outside = np.nonzero(m == 0)[0]
    j, t = np.meshgrid(np.arange(n_out), np.arange(6), indexing="ij")
    return _assemble(kfs, n_points, ((j * 13 + t * 1997 + shift) % n_points).ravel(), outside[j.ravel()], m, rng.integers(200, 1500, n_kf))


def word_edge(cols):
    """One bitmap word holds 32 columns: column counts 31 / 32 / 33 / 63 / 64 / 65 put the last column at bit 30 / 31 / 0 of the
    last word.  One window KeyFrame (id 1) with `cols` valid slots of distinct points and three invalid ones; outside KeyFrame 0
    observes exactly the last column, 2 every column, 3 nothing, 4 every other column."""
    rng = np.random.Generator(np.random.PCG64(5000 + cols))
    n_points = cols + 4
    pts = np.full(cols + 3, -1)
    at = np.sort(rng.choice(cols + 3, cols, replace=False))
    pts[at] = rng.permutation(n_points)[:cols]
    col_pts = pts[at]
    op = np.concatenate([col_pts[-1:], col_pts, col_pts[::2]])
    ok = np.concatenate([[0], np.full(cols, 2), np.full(len(col_pts[::2]), 4)])
    return _assemble([(pts, np.sort(rng.integers(0, 12, cols + 3)))], n_points, op, ok, _in_window(5, (1,)), [300, 400, 500, 600, 700])


def duplicates():
    """The reference adds a term per slot (MapSparsification.cc:100-107): a point held by two slots opens its column once and
    appears twice in the cell row and in the KeyFrame row.  On the device `first[p] == s` opens the column, the terms are written
    per slot.  Window KeyFrame 0: point 7 twice in cell 0 and again in cell 1, point 9 twice in cell 1; KeyFrame 1: 9 and 7 again,
    point 11 twice in cell 5; KeyFrames 2 and 3 draw 700 and 333 slots WITH replacement from 150 points over 20 cells."""
    rng = np.random.Generator(np.random.PCG64(6001))
    n_points, n_kf = 160, 7
    kfs = [([7, 7, 3, 7, 9, -1, 9, 2], [0, 0, 0, 1, 1, 1, 1, 6]), ([9, 7, 11, 11, -1], [0, 0, 5, 5, 9]),
           _random_kf(rng, 700, 150, 20, 0.85, replace=True), _random_kf(rng, 333, 150, 20, 0.85, replace=True)]
    m = _in_window(n_kf, (1, 2, 4, 5))
    op, ok = _random_outside(rng, n_points, np.nonzero(m == 0)[0], 2.0)
    return _assemble(kfs, n_points, op, ok, m, rng.integers(200, 1500, n_kf))


def sparse_validity():
    """Shapes of validity that an even spread never gives.  Window KeyFrames in order: 0 ordinary; 1 without slots; 2 ordinary; 3
    with 40 slots, all invalid (a KeyFrame row without terms, no cell row); 4 with a cell of 3000 slots valid only at its last (the
    look-back of first_valid runs 2999 slots), a cell of 50 valid only at its first, a cell of 20 without a valid slot, a cell of 3
    all valid; 5 with 5 slots (fewer than the 1024 threads of its workgroup); 6 with 2500 (three slots a thread, threads without
    any at the end)."""
    rng = np.random.Generator(np.random.PCG64(7001))
    n_points, n_kf = 3000, 12
    e_pts = np.full(3073, -1)
    e_pts[[2999, 3000, 3070, 3071, 3072]] = [41, 42, 43, 44, 45]
    e_cells = np.repeat([4, 9, 11, 12], [3000, 50, 20, 3])
    kfs = [_random_kf(rng, 50, n_points, 30), (np.zeros(0, int), np.zeros(0, int)), _random_kf(rng, 60, n_points, 30),
           (np.full(40, -1), np.sort(rng.integers(0, 30, 40))), (e_pts, e_cells), ([5, -1, 41, 6, -1], [2, 2, 3, 8, 8]),
           _random_kf(rng, 2500, n_points, valid=0.5)]
    m = _in_window(n_kf, (0, 2, 3, 5, 6, 8, 9))
    op, ok = _random_outside(rng, n_points, np.nonzero(m == 0)[0], 3.0)
    return _assemble(kfs, n_points, op, ok, m, rng.integers(200, 1500, n_kf))


def degenerate():
    """Windows at the ends of the argument ranges -> name: window.  All share 3 window KeyFrames x 60 slots, 10 KeyFrames, 100
    points unless the name says otherwise."""
    def base(seed, ids=(2, 5, 6), n_kf=10, outside_obs=True, **kw):
        rng = np.random.Generator(np.random.PCG64(8000 + seed))
        kfs = [_random_kf(rng, 60, 100, 25, 0.8) for _ in ids]
        m = _in_window(n_kf, ids)
        outside = np.nonzero(m == 0)[0]
        op, ok = _random_outside(rng, 100, outside, 3.0) if outside_obs and len(outside) else (np.zeros(0, int), np.zeros(0, int))
        return _assemble(kfs, 100, op, ok, m, rng.integers(200, 1500, n_kf), **kw)
    out = {}
    out["no_window_kf"] = base(1, ids=())                                  # n_window_kf == 0: no slot, no column, no row
    out["all_in_window"] = base(2, ids=(0, 1, 2), n_kf=3)                  # no KeyFrame outside: no bitmap, no kind-2 row
    out["no_observations"] = base(3, outside_obs=False, window_obs=False,  # n_obs == 0 with 7 KeyFrames outside
                                  point_nobs=np.random.Generator(np.random.PCG64(8003)).integers(1, 20, 100))
    w = base(4)
    true_max = int(w["point_nobs"][w["slot_point"][w["slot_point"] >= 0]].max())
    out["floor_below"] = dict(w, n_max_obs_floor=true_max - 1)             # the slots decide n_max_obs
    out["floor_above"] = dict(w, n_max_obs_floor=true_max + 5)             # the floor decides it, and every obj_coef
    w = base(5)
    w["kf_num_mps"][0] = 0                                                 # KeyFrame 0 is outside and observed: count / 0 = inf
    out["zero_num_mps"] = w
    out["N_zero"] = dict(base(6), N=0)                                     # every KeyFrame-row rhs is 0
    return out


def edge_windows():
    """name -> window, in the order the device tests run them."""
    out = {"scan_carry_%d" % n: scan_carry(n) for n in (1023, 1024, 1025, 2049)}
    out["many_slots"] = many_slots()
    out.update(("lds_hist_edge_%d" % n, lds_hist_edge(n)) for n in (LDS_HIST, LDS_HIST + 1))
    out["init_stride_dirty"] = init_stride(5)
    out["init_stride"] = init_stride()
    out.update(("word_edge_%d" % c, word_edge(c)) for c in (31, 32, 33, 63, 64, 65))
    out["duplicates"] = duplicates()
    out["sparse_validity"] = sparse_validity()
    out.update(("degenerate_" + k, v) for k, v in degenerate().items())
    return out


# cases whose point is what an earlier call left in the calling thread's grow-only scratch: run that one first, on the same thread
RUN_AFTER = {"init_stride": "init_stride_dirty"}
