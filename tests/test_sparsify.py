"""MapSparsification constraint-matrix assembly: oracle properties (CPU) and device parity (GPU)."""
import os
import re

import numpy as np
import pytest

import sparsify_cases as sc

KEYS = ("col_point", "obj_coef", "row_begin", "row_kind", "row_owner", "row_rhs", "col_idx")


def test_oracle_matrix_properties(oracle):
    w = sc.window(1, n_window=10, n_outside=30, n_points=2000, slots_per_kf=600)
    m = oracle.visibility_csr(N=100, **w)
    sp = w["slot_point"]
    valid = sp[sp >= 0]
    # columns: unique valid points in first-encounter order
    _, first = np.unique(valid, return_index=True)
    assert np.array_equal(m["col_point"], valid[np.sort(first)])
    assert m["n_max_obs"] == w["point_nobs"][valid].max()
    assert np.array_equal(m["obj_coef"], (m["n_max_obs"] - w["point_nobs"][m["col_point"]]).astype(np.float32))
    kinds = m["row_kind"]
    assert (kinds == 1).sum() == 10                                   # one row per window keyframe, rhs N
    assert np.all(m["row_rhs"][kinds == 1] == 100) and np.all(m["row_rhs"][kinds == 0] == 1)
    # keyframe row = concatenation of its cell rows
    r = 0
    for k in range(10):
        cells = []
        while kinds[r] == 0:
            cells.append(m["col_idx"][m["row_begin"][r]:m["row_begin"][r + 1]]); r += 1
        kf = m["col_idx"][m["row_begin"][r]:m["row_begin"][r + 1]]
        assert np.array_equal(np.concatenate(cells) if cells else np.zeros(0, np.int32), kf)
        assert len(kf) == (sp[w["kf_slot_begin"][k]:w["kf_slot_begin"][k + 1]] >= 0).sum()
        r += 1
    # outside rows: ascending keyframe id, rhs = count/total*N in float
    ext = np.nonzero(kinds == 2)[0]
    assert np.all(np.diff(m["row_owner"][ext]) > 0) and not w["kf_in_window"][m["row_owner"][ext]].any()
    for r in ext[:20]:
        cols = m["col_idx"][m["row_begin"][r]:m["row_begin"][r + 1]]
        kf = m["row_owner"][r]
        assert np.all(np.diff(cols) > 0)
        want = [c for c, p in enumerate(m["col_point"]) if kf in w["obs_kf"][w["obs_begin"][p]:w["obs_begin"][p + 1]]]
        assert cols.tolist() == want
        assert m["row_rhs"][r] == np.float32(np.float32(len(cols)) / np.float32(w["kf_num_mps"][kf])) * np.float32(100)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,kw", [(1, {}), (2, dict(n_window=3, n_outside=0, n_points=500, slots_per_kf=300)),
                                     (3, dict(n_window=30, n_outside=200, n_points=20000, slots_per_kf=2000, tracked_frac=0.9)),
                                     (4, dict(n_window=1, n_outside=5, n_points=50, slots_per_kf=40, tracked_frac=0.0))])
def test_device_matrix_matches_oracle(msorb_mod, oracle, seed, kw):
    w = sc.window(seed, **kw)
    got = msorb_mod.visibility_csr(N=100, **w)
    want = oracle.visibility_csr(N=100, **w)
    assert (got["n_cols"], got["n_rows"], got["n_max_obs"]) == (want["n_cols"], want["n_rows"], want["n_max_obs"])
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------
# Structural cases (sparsify_cases.edge_windows): three independent statements of MapSparsification.cc:58-151 — the plain
# reference in sparsify_cases.py, the C++ oracle, the device — have to agree byte for byte; DESIGN.md §22.
# ------------------------------------------------------------------------------------------------
EDGE = sc.edge_windows()
RANDOM = {"random_%d" % seed: (seed, kw) for seed, kw in
          [(1, {}), (2, dict(n_window=3, n_outside=0, n_points=500, slots_per_kf=300)),
           (3, dict(n_window=30, n_outside=200, n_points=20000, slots_per_kf=2000, tracked_frac=0.9)),
           (4, dict(n_window=1, n_outside=5, n_points=50, slots_per_kf=40, tracked_frac=0.0))]}
_cache = {}


def _case(name):
    """(arrays, N, floor, plain reference) of a case, computed once and shared"""
    if name not in _cache:
        w = EDGE[name] if name in EDGE else sc.window(RANDOM[name][0], **RANDOM[name][1])
        arrays, N, floor = sc.split(w)
        _cache[name] = (arrays, N, floor, sc.reference_csr(arrays, N, floor))
    return _cache[name]


def _rows(m, kind):
    """{owner: column list} of the rows of one kind"""
    rb, ci = m["row_begin"], m["col_idx"]
    return {int(m["row_owner"][r]): ci[rb[r]:rb[r + 1]] for r in np.nonzero(m["row_kind"] == kind)[0]}


def test_case_constants_match_the_kernels():
    """The sizes of the cases come from these constants of csrc/visibility.hip; a change there has to be followed in sparsify_cases.py."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ms-slam_amd", "csrc", "visibility.hip")).read()
    assert re.search(r"constexpr int kLdsHist = (\d+);", src).group(1) == str(sc.LDS_HIST)
    assert "const bool lds = n_kf <= kLdsHist;" in src and "n_kf_total <= kLdsHist ? (size_t)n_kf_total * sizeof(int) : 0" in src
    assert re.search(r"constexpr int kKfThreads = (\d+);", src).group(1) == str(sc.KF_THREADS)
    assert "for (int base = 0; base < n_kf; base += %d)" % sc.SCAN_CHUNK in src
    assert "vis_extra_scan_kernel, dim3(1), dim3(%d)" % sc.SCAN_CHUNK in src
    assert "for (int i = threadIdx.x; i < (int)blockIdx.x; i += %d) part += block_base[i];" % sc.COLUMNS_BLOCK in src
    assert "const int s = blockIdx.x * %d + threadIdx.x;" % sc.COLUMNS_BLOCK in src
    assert "std::min<size_t>((n_init + 255) / 256, %d)), dim3(%d)" % (sc.INIT_GRID, sc.COLUMNS_BLOCK) in src


@pytest.mark.parametrize("name", list(EDGE) + list(RANDOM))
def test_oracle_equals_plain_reference(oracle, name):
    arrays, N, floor, ref = _case(name)
    assert sc.csr_differences(oracle.visibility_csr(N=N, n_max_obs_floor=floor, **arrays), ref) == []


@pytest.mark.parametrize("n_kf", [1023, 1024, 1025, 2049])
def test_scan_carry_reaches_every_chunk(n_kf):
    w, _, _, ref = _case("scan_carry_%d" % n_kf)
    assert len(w["kf_in_window"]) == n_kf and w["kf_in_window"].sum() == 2
    counted = np.zeros(n_kf, bool)
    counted[list(_rows(ref, 2))] = True
    assert counted[n_kf - 1] and not counted.all()              # the last KeyFrame has a row; ranks differ from indices
    chunks = [counted[b:b + sc.SCAN_CHUNK] for b in range(0, n_kf, sc.SCAN_CHUNK)]
    assert len(chunks) == -(-n_kf // sc.SCAN_CHUNK) and all(c.any() for c in chunks)
    for edge in range(sc.SCAN_CHUNK, n_kf + 1, sc.SCAN_CHUNK):  # both sides of every chunk boundary
        assert counted[edge - 1] and (edge >= n_kf or counted[edge])
    if n_kf > sc.SCAN_CHUNK:                                    # what the carries hold when the last trip starts
        last = (n_kf - 1) // sc.SCAN_CHUNK * sc.SCAN_CHUNK
        assert counted[:last].sum() > 0 and sum(len(c) for kf, c in _rows(ref, 2).items() if kf < last) > 0


def test_many_slots_has_first_encounters_beyond_block_256():
    w, _, _, ref = _case("many_slots")
    sp = w["slot_point"]
    assert len(sp) > 65536 and (len(sp) - 1) // sc.COLUMNS_BLOCK > sc.COLUMNS_BLOCK
    slots = np.nonzero(sp >= 0)[0]
    _, at = np.unique(sp[slots], return_index=True)
    first = np.sort(slots[at])                                  # the slots that open a column
    assert np.array_equal(ref["col_point"], sp[first])
    block = first // sc.COLUMNS_BLOCK
    assert (block == sc.COLUMNS_BLOCK).any()                    # a non-zero count at index 256: the first value of a second trip
    assert (block > sc.COLUMNS_BLOCK).sum() > 50                # ranks that depend on the second trip
    assert np.diff(w["kf_slot_begin"]).max() > sc.KF_THREADS    # more than one slot per thread of a KeyFrame's workgroup


@pytest.mark.parametrize("n_kf", [sc.LDS_HIST, sc.LDS_HIST + 1])
def test_lds_hist_edge_counts_at_the_last_keyframe(n_kf):
    w, _, _, ref = _case("lds_hist_edge_%d" % n_kf)
    assert len(w["kf_in_window"]) == n_kf and w["obs_kf"].max() == n_kf - 1
    rows = _rows(ref, 2)
    assert all(len(rows[kf]) > 100 for kf in (0, sc.LDS_HIST - 1, n_kf - 2, n_kf - 1))
    assert 1500 < ref["n_cols"] < 2500


def _bitmap_words(w):
    n_valid = int((w["slot_point"] >= 0).sum())
    return -(-min(n_valid, len(w["point_nobs"])) // 32), int((w["kf_in_window"] == 0).sum())


def test_init_stride_sets_bits_beyond_the_first_trip():
    w, _, _, ref = _case("init_stride")
    words, n_outside = _bitmap_words(w)
    one_trip = sc.INIT_GRID * sc.COLUMNS_BLOCK
    assert one_trip == 524288 and n_outside * words > one_trip
    def words_set(m):
        rows = _rows(m, 2)
        return {rank * words + int(c) // 32 for rank, kf in enumerate(sorted(rows)) for c in rows[kf]}
    mine = words_set(ref)
    assert sum(x >= one_trip for x in mine) > 100 and min(mine) < 1000
    # the call in front of it has the same scratch layout (every array as long) and leaves other words beyond the first trip set
    dirty, _, _, dirty_ref = _case(sc.RUN_AFTER["init_stride"])
    assert all(dirty[k].shape == w[k].shape for k in w) and np.array_equal(dirty["slot_point"], w["slot_point"])
    assert sum(x >= one_trip for x in words_set(dirty_ref) - mine) > 100


@pytest.mark.parametrize("cols", [31, 32, 33, 63, 64, 65])
def test_word_edge_columns(cols):
    w, _, _, ref = _case("word_edge_%d" % cols)
    assert ref["n_cols"] == cols and _bitmap_words(w)[0] == -(-cols // 32)
    rows = _rows(ref, 2)
    assert sorted(rows) == [0, 2, 4] and rows[0].tolist() == [cols - 1] and rows[2].tolist() == list(range(cols))


def test_duplicates_are_kept_as_terms():
    w, _, _, ref = _case("duplicates")
    sp, cell, ksb = w["slot_point"], w["slot_cell"], w["kf_slot_begin"]
    kf_of = np.repeat(np.arange(len(ksb) - 1), np.diff(ksb))
    v = sp >= 0
    triples = np.stack([kf_of[v], cell[v], sp[v]], 1)
    assert len(np.unique(triples, axis=0)) < len(triples)                             # a point twice in one cell
    pairs = np.unique(triples, axis=0)[:, [0, 2]]
    assert len(np.unique(pairs, axis=0)) < len(pairs)                                 # ... in two cells of one KeyFrame
    assert np.bincount(np.unique(triples[:, [0, 2]], axis=0)[:, 1]).max() == 4        # ... in every KeyFrame
    assert len(np.unique(ref["col_point"])) == ref["n_cols"] == len(np.unique(sp[v])) # its column opens once
    kf_rows, cell_terms = _rows(ref, 1), 0
    for k in range(len(ksb) - 1):                                                     # every slot is a term, twice
        assert len(kf_rows[k]) == v[ksb[k]:ksb[k + 1]].sum() > len(np.unique(kf_rows[k]))
    rb = ref["row_begin"]
    for r in np.nonzero(ref["row_kind"] == 0)[0]:
        cell_terms += rb[r + 1] - rb[r]
    assert cell_terms == v.sum()
    assert ref["col_idx"][:3].tolist() == [0, 0, 1]                                   # cell 0 of KeyFrame 0: points 7, 7, 3


def test_sparse_validity_shapes():
    w, _, _, ref = _case("sparse_validity")
    sp, cell, ksb = w["slot_point"], w["slot_cell"], w["kf_slot_begin"]
    n = np.diff(ksb)
    assert n.tolist()[1] == 0 and n[0] > 0 and n[2] > 0                               # no slots, between two others
    assert n[3] > 0 and (sp[ksb[3]:ksb[4]] < 0).all() and len(_rows(ref, 1)[3]) == 0  # all invalid: a row without terms
    e = slice(ksb[4], ksb[5])
    run = np.nonzero(cell[e] == 4)[0]
    assert len(run) == 3000 and (sp[e][run[:-1]] < 0).all() and sp[e][run[-1]] >= 0   # valid only at its last slot
    run = np.nonzero(cell[e] == 9)[0]
    assert (sp[e][run[1:]] < 0).all() and sp[e][run[0]] >= 0                          # valid only at its first
    assert n[5] == 5 < sc.KF_THREADS and n[6] == 2500 > 2 * sc.KF_THREADS
    kinds = ref["row_kind"].tolist()                                                  # KeyFrame 4 has cell rows 4, 9, 12 and not 11
    r4 = [i for i, k in enumerate(kinds) if k == 1][4]
    assert kinds[r4 - 3:r4] == [0, 0, 0] and ref["row_owner"][r4 - 3:r4].tolist() == [4, 9, 12] and kinds[r4 - 4] == 1


def test_degenerate_windows_are_what_they_say():
    g = lambda name: _case("degenerate_" + name)
    w, _, _, ref = g("no_window_kf")
    assert len(w["kf_slot_begin"]) == 1 and len(w["obs_kf"]) > 0 and (ref["n_rows"], ref["n_cols"], len(ref["col_idx"])) == (0, 0, 0)
    w, _, _, ref = g("all_in_window")
    assert w["kf_in_window"].all() and len(w["obs_kf"]) > 0 and not (ref["row_kind"] == 2).any()
    w, _, _, ref = g("no_observations")
    assert len(w["obs_kf"]) == 0 and (w["kf_in_window"] == 0).sum() == 7 and not (ref["row_kind"] == 2).any() and ref["n_cols"] > 0
    (w, _, lo, below), (_, _, hi, above) = g("floor_below"), g("floor_above")
    true_max = int(w["point_nobs"][w["slot_point"][w["slot_point"] >= 0]].max())
    assert 0 < lo < true_max == below["n_max_obs"] < hi == above["n_max_obs"]
    assert np.array_equal(above["obj_coef"] - below["obj_coef"], np.full(below["n_cols"], hi - true_max, np.float32))
    w, _, _, ref = g("zero_num_mps")
    rhs = ref["row_rhs"][ref["row_kind"] == 2]
    assert w["kf_num_mps"][0] == 0 and np.isinf(rhs[0]) and rhs[0] > 0 and np.isfinite(rhs[1:]).all() and len(rhs) > 1
    _, N, _, ref = g("N_zero")
    assert N == 0 and (ref["row_kind"] == 2).any() and np.all(ref["row_rhs"][ref["row_kind"] != 0] == 0)


def _three_way(msorb_mod, oracle, name):
    arrays, N, floor, ref = _case(name)
    got = msorb_mod.visibility_csr(N=N, n_max_obs_floor=floor, **arrays)
    want = oracle.visibility_csr(N=N, n_max_obs_floor=floor, **arrays)
    diff = dict(device_vs_reference=sc.csr_differences(got, ref), device_vs_oracle=sc.csr_differences(got, want),
                oracle_vs_reference=sc.csr_differences(want, ref))
    assert not any(diff.values()), (name, diff)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EDGE))
def test_device_equals_reference_and_oracle(msorb_mod, oracle, name):
    if name in sc.RUN_AFTER:
        _three_way(msorb_mod, oracle, sc.RUN_AFTER[name])
    _three_way(msorb_mod, oracle, name)


@pytest.mark.gpu
def test_scratch_reuse_order(msorb_mod, oracle):
    """The scratch of a calling thread only grows and is not cleared between calls: after the largest case every small one has to
    come out as if it were the first (stale bitmap words, first[] marks, counters and scalars would show here)."""
    largest = max(EDGE, key=lambda n: sum(a.nbytes for a in EDGE[n].values() if isinstance(a, np.ndarray)))
    assert largest == "many_slots"
    order = [largest] + [n for n in EDGE if n.startswith("degenerate_")] + [n for n in EDGE if n.startswith("word_edge_")]
    for name in order + [largest]:
        _three_way(msorb_mod, oracle, name)


@pytest.mark.gpu
def test_many_slots_is_repeatable(msorb_mod):
    arrays, N, floor, ref = _case("many_slots")
    a = msorb_mod.visibility_csr(N=N, n_max_obs_floor=floor, **arrays)
    b = msorb_mod.visibility_csr(N=N, n_max_obs_floor=floor, **arrays)
    assert sc.csr_differences(a, b) == [] and sc.csr_differences(a, ref) == []


@pytest.mark.gpu
@pytest.mark.parametrize("short", [None, "cols", "rows", "nnz"])
def test_capacity_through_the_c_abi(msorb_mod, short):
    """Exact capacities succeed; one short in any of the three is MSORB_E_CAPACITY and leaves the caller's memory as it was."""
    import ctypes as C
    arrays, N, floor, ref = _case("duplicates")
    L, p = msorb_mod.lib(), msorb_mod._np_ptr
    L.msorb_visibility_csr.argtypes = ([C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int] +
                                       [C.c_void_p] * 2 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int] +
                                       [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3)
    cap = dict(cols=ref["n_cols"], rows=ref["n_rows"], nnz=len(ref["col_idx"]))
    assert min(cap.values()) > 1
    if short:
        cap[short] -= 1
    fill = lambda n, dt: np.frombuffer(bytes([0xAB]) * (n * 4), dt).copy()
    out = dict(col_point=fill(cap["cols"], np.int32), obj_coef=fill(cap["cols"], np.float32), row_begin=fill(cap["rows"] + 1, np.int32),
               row_kind=fill(cap["rows"], np.int32), row_owner=fill(cap["rows"], np.int32), row_rhs=fill(cap["rows"], np.float32),
               col_idx=fill(cap["nnz"], np.int32))
    counts = fill(4, np.int32)                                   # n_cols, n_rows, nnz, n_max_obs
    before = {k: v.tobytes() for k, v in out.items()}
    a = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    cp = lambda i: counts[i:i + 1].ctypes.data
    rc = L.msorb_visibility_csr(0, len(a["kf_slot_begin"]) - 1, p(a["kf_slot_begin"]), p(a["slot_point"]), p(a["slot_cell"]),
                                len(a["point_nobs"]), p(a["point_nobs"]), p(a["obs_begin"]), p(a["obs_kf"]), len(a["kf_in_window"]),
                                p(a["kf_in_window"]), p(a["kf_num_mps"]), N, floor, cp(0), p(out["col_point"]), cap["cols"], cp(1),
                                p(out["row_begin"]), p(out["row_kind"]), p(out["row_owner"]), p(out["row_rhs"]), cap["rows"],
                                p(out["col_idx"]), cap["nnz"], cp(2), p(out["obj_coef"]), cp(3))
    if short:
        assert rc == msorb_mod.E_CAPACITY
        assert {k: v.tobytes() for k, v in out.items()} == before and counts.tobytes() == bytes([0xAB]) * 16
    else:
        assert rc == 0
        assert counts.tolist() == [ref["n_cols"], ref["n_rows"], len(ref["col_idx"]), ref["n_max_obs"]]
        assert sc.csr_differences(dict(out, n_cols=counts[0], n_rows=counts[1], n_max_obs=counts[3]), ref) == []
