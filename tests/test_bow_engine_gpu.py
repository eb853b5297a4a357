"""The host engine of the BoW-node searches (ms-slam_amd/csrc/bow_match.hip: one merge walk, one block layout, one round trip behind
msorb_search_by_bow, _rig, msorb_search_for_triangulation, _cb and the two resident-KeyFrame forms) on the smallest shapes at which
the shared walk, layout or round trip can go wrong: about 130 features a side, common nodes whose train lists have 63, 64 and 65
entries (the 64-train chunks that size the kernels' LDS), a pair with no query features, a pair without a common node BETWEEN
pairs that have some (its items are missing from the list, its rows are not), FeatureVectors whose lists sit behind unused
entries (begin[0] > 0), a pair with every train available (avail2 = NULL).  Every entry is compared with the oracle, the batched
call with the single calls, the resident forms with the per-call ones.  The large shapes are in test_bow_match.py,
test_kf_store_gpu.py and test_matcher_rig_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import bow_match_cases as bmc

pytestmark = pytest.mark.gpu
SCALE = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
SIGMA2 = (SCALE * SCALE).astype(np.float32)


def _renode(p, sizes, lost=0.08, seed=0):
    """p's FeatureVectors rebuilt: set 2's first sum(sizes) features fill nodes 10, 13, ... with exactly `sizes` entries, the rest go
    to three more nodes; a set-1 feature goes to the node of its nearest train, or (`lost`) to a node set 2 does not have."""
    rng = np.random.default_rng(9000 + seed)
    n1, n2 = len(p["desc1"]), len(p["desc2"])
    node2 = 100 + 3 * rng.integers(0, 3, n2)
    node2[:sum(sizes)] = np.repeat(10 + 3 * np.arange(len(sizes)), sizes)
    perm = rng.permutation(n2)                                  # (the lists are not runs of consecutive features)
    inv = np.argsort(perm)
    node2 = node2[inv]
    if n1 and n2:
        bits1, bits2 = np.unpackbits(p["desc1"], axis=1).astype(np.int32), np.unpackbits(p["desc2"], axis=1).astype(np.int32)
        dist = bits1.sum(1)[:, None] + bits2.sum(1)[None, :] - 2 * bits1 @ bits2.T
        node1 = node2[dist.argmin(1)].copy()
    else:
        node1 = 10 + 3 * rng.integers(0, 3, n1)
    node1[rng.random(n1) < lost] = 11
    p["fv1"], p["fv2"] = bmc.feature_vector_from_nodes(node1), bmc.feature_vector_from_nodes(node2)
    for fv in (p["fv1"], p["fv2"]):
        for r in range(len(fv[0])):
            rng.shuffle(fv[2][fv[1][r]:fv[1][r + 1]])
    return p


def _behind(fv, k):
    """the same FeatureVector with its lists behind k unused entries of feat"""
    return fv[0], (fv[1] + k).astype(np.int32), np.concatenate([np.zeros(k, np.int32), fv[2]]).astype(np.int32)


def _list_sizes(fv1, fv2):
    both = np.intersect1d(fv1[0], fv2[0])
    return sorted(int(fv2[1][r + 1] - fv2[1][r]) for r in np.flatnonzero(np.isin(fv2[0], both)))


@pytest.fixture(scope="module")
def bow_set():
    ps = [_renode(bmc.make_pair(700, n1=130, n2=130, flip=30, dup_frac=0.2), [63, 64, 3], seed=0),
          _renode(bmc.make_pair(701, n1=0, n2=130), [40], seed=1),
          _renode(bmc.make_pair(702, n1=129, n2=131, flip=30, dup_frac=0.2), [65, 40], seed=2),
          _renode(bmc.make_pair(703, n1=131, n2=128), [50, 50], seed=3),
          _renode(bmc.make_pair(704, n1=130, n2=133, flip=30), [64, 65], seed=4),
          _renode(bmc.make_pair(705, n1=127, n2=130, flip=30), [63, 30], seed=5)]
    ps[3]["fv1"] = (ps[3]["fv1"][0] + 1, ps[3]["fv1"][1], ps[3]["fv1"][2])          # no common node
    ps[4]["fv1"], ps[4]["fv2"] = _behind(ps[4]["fv1"], 5), _behind(ps[4]["fv2"], 3)
    ps[5]["avail2"] = None
    assert {63, 64}.issubset(_list_sizes(ps[0]["fv1"], ps[0]["fv2"])) and 65 in _list_sizes(ps[2]["fv1"], ps[2]["fv2"])
    assert len(np.intersect1d(ps[3]["fv1"][0], ps[3]["fv2"][0])) == 0 and ps[4]["fv1"][1][0] == 5 and ps[4]["fv2"][1][0] == 3
    return ps


def _search_by_bow(msorb, pairs, th_low, inclusive, nnratio, ori, timed):
    """msorb_search_by_bow through ctypes, with or without the elapsed_ms pointer (msorb.search_by_bow always passes one)"""
    lb = msorb.lib()
    lb.msorb_search_by_bow.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]
    arr = (msorb.BowPair * len(pairs))()
    keep, outs = [], []
    for q, p in zip(arr, pairs):
        fv = [np.ascontiguousarray(a, np.int32) for a in (*p["fv1"], *p["fv2"])]
        m12, m21 = np.full(max(len(p["desc1"]), 1), 7, np.int32), np.full(max(len(p["desc2"]), 1), 7, np.int32)
        keep.append(fv)
        outs.append((m12[:len(p["desc1"])], m21[:len(p["desc2"])]))
        q.n1, q.n2 = len(p["desc1"]), len(p["desc2"])
        q.desc1, q.desc2, q.valid1 = (p[k].ctypes.data for k in ("desc1", "desc2", "valid1"))
        q.avail2 = None if p["avail2"] is None else p["avail2"].ctypes.data
        q.fv1_nodes, q.fv1_node, q.fv1_begin, q.fv1_feat = len(fv[0]), *(a.ctypes.data for a in fv[:3])
        q.fv2_nodes, q.fv2_node, q.fv2_begin, q.fv2_feat = len(fv[3]), *(a.ctypes.data for a in fv[3:])
        q.angle1, q.angle2, q.match12, q.match21 = p["angle1"].ctypes.data, p["angle2"].ctypes.data, m12.ctypes.data, m21.ctypes.data
    ms = C.c_float(-1.0)
    rc = lb.msorb_search_by_bow(0, C.addressof(arr), len(pairs), th_low, int(inclusive), nnratio, int(ori), C.addressof(ms) if timed else None)
    assert rc == 0, msorb.last_error() if hasattr(msorb, "last_error") else rc
    assert (ms.value > 0) if timed else (ms.value == -1.0)
    return [(q.nmatches, o[0].tolist(), o[1].tolist()) for q, o in zip(arr, outs)]


CONFIGS = [(50, True, 0.7, True), (50, False, 0.8, False)]


@pytest.fixture(scope="module")
def bow_want(bow_set, oracle):
    want = {}
    for cfg in CONFIGS:
        th, inc, ratio, ori = cfg
        want[cfg] = []
        for p in bow_set:
            nm, m12, m21 = oracle.search_by_bow(p["desc1"], p["desc2"], p["valid1"], p["avail2"], p["fv1"], p["fv2"], p["angle1"], p["angle2"],
                                                th, inc, ratio, ori)
            want[cfg].append((int(nm), m12.tolist(), m21.tolist()))
    # the set exercises what it is meant to: matches in the pairs with common nodes, none elsewhere, the rotation filter withdraws some
    nm = [w[0] for w in want[CONFIGS[0]]]
    assert min(nm[0], nm[2], nm[4], nm[5]) > 20 and nm[1] == 0 and nm[3] == 0
    assert sum(w[0] for w in want[CONFIGS[1]]) != sum(nm)
    return want


@pytest.mark.parametrize("timed", [True, False], ids=["elapsed", "no_elapsed"])
def test_per_call_batched_and_single_equal_the_oracle(msorb_mod, bow_set, bow_want, timed):
    for cfg in CONFIGS:
        batched = _search_by_bow(msorb_mod, bow_set, *cfg, timed)
        assert batched == bow_want[cfg], cfg
        for p, w in zip(bow_set, bow_want[cfg]):
            if len(p["desc1"]) and len(np.intersect1d(p["fv1"][0], p["fv2"][0])):   # (a call that launches: the others report no time)
                assert _search_by_bow(msorb_mod, [p], *cfg, timed) == [w], cfg
            else:
                assert _search_by_bow(msorb_mod, [p], *cfg, False) == [w], cfg


def _kps(n, angle):
    k = np.zeros(n, bmc.KP_DTYPE)
    k["angle"] = angle
    return k


def test_resident_forms_equal_the_per_call_results(msorb_mod, bow_set, bow_want):
    st = msorb_mod.KeyFrameStore()
    try:
        id1 = [st.add(_kps(len(p["desc1"]), p["angle1"]), p["desc1"], p["fv1"], SCALE, SIGMA2) for p in bow_set]
        id2 = [st.add(_kps(len(p["desc2"]), p["angle2"]), p["desc2"], p["fv2"], SCALE, SIGMA2) for p in bow_set]
        for cfg in CONFIGS:
            # KeyFrame trains: the whole set in one call
            got, _ = st.search_by_bow([dict(kf1=a, kf2=b, valid1=p["valid1"], avail2=p["avail2"]) for a, b, p in zip(id1, id2, bow_set)],
                                      None, *cfg)
            assert [(g[0], g[1].tolist(), g[2].tolist()) for g in got] == bow_want[cfg], cfg
            # frame trains: every pair's set 2 as the frame of a call (pair 4's lists sit behind 3 unused entries)
            for a, p, w in zip(id1, bow_set, bow_want[cfg]):
                frame = dict(desc=p["desc2"], fv=p["fv2"], angle=p["angle2"])
                got, _ = st.search_by_bow([dict(kf1=a, kf2=-1, valid1=p["valid1"], avail2=p["avail2"])], frame, *cfg)
                assert (got[0][0], got[0][1].tolist(), got[0][2].tolist()) == w, cfg
        # frame trains, several KeyFrames against one frame whose lists sit behind unused entries: the KeyFrame without features, the
        # one stored from a vector with begin[0] > 0 and one whose nodes the frame does not have in between
        f = bow_set[4]
        frame = dict(desc=f["desc2"], fv=f["fv2"], angle=f["angle2"])
        order = [0, 1, 4, 3, 2]
        ref = [dict(bow_set[i], desc2=f["desc2"], fv2=f["fv2"], angle2=f["angle2"], avail2=None) for i in order]
        got, _ = st.search_by_bow([dict(kf1=id1[i], kf2=-1, valid1=bow_set[i]["valid1"]) for i in order], frame, *CONFIGS[0])
        want = _search_by_bow(msorb_mod, ref, *CONFIGS[0], True)
        assert [(g[0], g[1].tolist(), g[2].tolist()) for g in got] == want
        assert want[2][0] > 20 and want[1][0] == 0 and want[3][0] == 0
    finally:
        st.close()


# ---- SearchForTriangulation: per call, resident, and with the geometric test handed in by the caller ---------------------------
@pytest.fixture(scope="module")
def tri_set():
    ps = [_renode(bmc.make_triangulation_pair(710, n1=130, n2=130, n_nodes=4), [63, 64, 3], lost=0.05, seed=10),
          _renode(bmc.make_triangulation_pair(711, n1=0, n2=130, n_nodes=4), [40], seed=11),
          _renode(bmc.make_triangulation_pair(712, n1=129, n2=131, n_nodes=4), [65, 40], lost=0.05, seed=12),
          _renode(bmc.make_triangulation_pair(713, n1=131, n2=128, n_nodes=4), [50, 50], seed=13),
          _renode(bmc.make_triangulation_pair(714, n1=130, n2=133, n_nodes=4), [64, 65], lost=0.05, seed=14)]
    ps[3]["fv1"] = (ps[3]["fv1"][0] + 1, ps[3]["fv1"][1], ps[3]["fv1"][2])
    ps[4]["fv1"], ps[4]["fv2"] = _behind(ps[4]["fv1"], 4), _behind(ps[4]["fv2"], 6)
    assert {63, 64}.issubset(_list_sizes(ps[0]["fv1"], ps[0]["fv2"])) and 65 in _list_sizes(ps[2]["fv1"], ps[2]["fv2"])
    return ps


def _epipolar_gate(p, coarse):
    """the per-call entry's test of a (query, train) as the caller of msorb_search_for_triangulation_cb would state it: the epipole
    distance of ORBmatcher.cc:1283-1291 and Pinhole::epipolarConstrain (Pinhole.cpp:107-131), in float32 steps"""
    f32, f64 = np.float32, np.float64
    F, ep = p["F12"].reshape(3, 3).astype(f32), p["ep"].astype(f32)

    def fma(a, b, c):
        return f32(f64(a) * f64(b) + f64(c))

    def accept(i1, i2):
        x1, y1, x2, y2 = (f32(v) for v in (p["kp1"]["x"][i1], p["kp1"]["y"][i1], p["kp2"]["x"][i2], p["kp2"]["y"][i2]))
        octave = p["kp2"]["octave"][i2]
        if not p["stereo1"][i1] and not p["stereo2"][i2]:
            ex, ey = f32(ep[0] - x2), f32(ep[1] - y2)
            if fma(ex, ex, f32(ey * ey)) < f32(f32(100) * p["scale_factors2"][octave]):
                return False
        if coarse:
            return True
        a = f32(fma(x1, F[0, 0], f32(y1 * F[1, 0])) + F[2, 0])
        b = f32(fma(x1, F[0, 1], f32(y1 * F[1, 1])) + F[2, 1])
        c = f32(fma(x1, F[0, 2], f32(y1 * F[1, 2])) + F[2, 2])
        num, den = f32(fma(a, x2, f32(b * y2)) + c), fma(a, a, f32(b * b))
        return bool(den != 0 and f64(f32(f32(num * num) / den)) < 3.84 * f64(p["level_sigma2_2"][octave]))
    return accept


def test_triangulation_per_call_resident_and_callback_equal_the_oracle(msorb_mod, oracle, tri_set):
    st = msorb_mod.KeyFrameStore()
    try:
        id1 = [st.add(p["kp1"], p["desc1"], p["fv1"], SCALE, SIGMA2) for p in tri_set]
        id2 = [st.add(p["kp2"], p["desc2"], p["fv2"], p["scale_factors2"], p["level_sigma2_2"]) for p in tri_set]
        for coarse, ori in ((False, True), (True, False)):
            want = [oracle.search_for_triangulation(p, coarse, ori) for p in tri_set]
            want = [(int(nm), m12.tolist()) for nm, m12 in want]
            assert min(want[0][0], want[2][0], want[4][0]) > 10 and want[1][0] == 0 and want[3][0] == 0
            got, ms = msorb_mod.search_for_triangulation(tri_set, coarse, ori)
            assert [(g[0], g[1].tolist()) for g in got] == want and ms > 0
            for p, w in zip(tri_set, want):
                one, _ = msorb_mod.search_for_triangulation([p], coarse, ori)
                assert (one[0][0], one[0][1].tolist()) == w
            got, _ = st.search_for_triangulation([dict(kf1=a, kf2=b, valid1=p["valid1"], avail2=p["avail2"], stereo1=p["stereo1"],
                                                       stereo2=p["stereo2"], F12=p["F12"], ep=p["ep"]) for a, b, p in zip(id1, id2, tri_set)],
                                                 coarse, ori)
            assert [(g[0], g[1].tolist()) for g in got] == want
            for p, w in zip(tri_set, want):
                q = dict(desc1=p["desc1"], desc2=p["desc2"], valid1=p["valid1"], avail2=p["avail2"], fv1=p["fv1"], fv2=p["fv2"],
                         angle1=p["kp1"]["angle"], angle2=p["kp2"]["angle"])
                nm, m12, calls = msorb_mod.search_for_triangulation_cb(q, _epipolar_gate(p, coarse), 50, ori)
                assert (nm, m12.tolist()) == w
                assert (len(calls) > 0) == (w[0] > 0)
    finally:
        st.close()
    # the rotation filter withdrew something in the first configuration (else the second leg of every form above was idle)
    plain = sum(int(oracle.search_for_triangulation(p, False, False)[0]) for p in tri_set)
    assert plain > sum(int(oracle.search_for_triangulation(p, False, True)[0]) for p in tri_set)


# ---- SearchByBoW(pKF, F) on a two-camera frame: two entries per KeyFrame feature into one histogram ----------------------------
@pytest.mark.parametrize("n_left", [0, 61, 130])
def test_rig_call_on_a_small_frame(msorb_mod, oracle, n_left):
    p = _renode(bmc.make_pair(720, n1=130, n2=130, flip=30, dup_frac=0.3), [63, 64, 3], seed=20)
    rng = np.random.default_rng(721)
    if 0 < n_left < 130:                                         # right-camera rows as near copies of left rows, in the same node
        node2 = np.zeros(130, np.int64)
        for r, nd in enumerate(p["fv2"][0]):
            node2[p["fv2"][2][p["fv2"][1][r]:p["fv2"][1][r + 1]]] = nd
        twin = np.arange(n_left, 130)[rng.random(130 - n_left) < 0.7]
        src = rng.integers(0, n_left, len(twin))
        p["desc2"][twin] = bmc.bow_cases._flip_bits(rng, p["desc2"][src], rng.integers(0, 10, len(twin)))
        p["angle2"][twin] = p["angle2"][src]
        node2[twin] = node2[src]
        p = _renode_keep1(p, node2)
    p["avail2"] = None
    for ratio, ori in ((0.7, True), (0.9, False)):
        wn, w21 = oracle.search_by_bow_rig(p, n_left, 50, ratio, ori)
        gn, g21, g12 = msorb_mod.search_by_bow_rig(p, n_left, 50, ratio, ori)
        assert gn == wn and g21.tolist() == w21.tolist(), (n_left, ratio, ori)
        assert (wn > 20) == (n_left > 0)                         # (without left features no right match is looked at, :330)
        left = np.flatnonzero(g12 >= 0)
        assert all(g12[k] < n_left and g21[g12[k]] == k for k in left) and len(left) == int((g21[:n_left] >= 0).sum())
    if 0 < n_left < 130:
        w21 = oracle.search_by_bow_rig(p, n_left, 50, 0.7, True)[1]
        assert len(set(w21[:n_left][w21[:n_left] >= 0]) & set(w21[n_left:][w21[n_left:] >= 0])) > 3   # features matched in both cameras


def _renode_keep1(p, node2):
    """set 2's FeatureVector from node2, set 1's kept"""
    p["fv2"] = bmc.feature_vector_from_nodes(node2)
    return p
