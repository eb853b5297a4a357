"""The case sets of tests/boundary_cases.py held to their purpose, on the CPU oracle alone: the logf read-out is valid for every
one of its cases, every boundary family holds both outcomes with its centre row ON the boundary, and every output field of
every kernel under test is observed with more than one value."""
import numpy as np
import pytest

import boundary_cases as bc


@pytest.fixture(scope="module")
def logf_set(oracle):
    c = bc.logf_cases(oracle)
    return c, bc.logf_points(c["ratio"], c["kexp"])


def test_flip_points_are_where_the_level_changes(oracle):
    """... and not always at 1.2f ** k: with logf(1.2f) they are, with the float above it the level changes elsewhere"""
    assert np.array_equal(oracle.logf_n(np.array([1.2, 2.0, 1.1], np.float32)), np.array(bc.log_scale_factors(), np.float32)[[0, 2, 3]])
    powers = np.ones(8, np.float32)
    for k in range(1, 8):
        powers[k] = powers[k - 1] * np.float32(1.2)
    lsf = bc.log_scale_factors()[1]
    flips = np.array([bc.flip_point(oracle, lsf, k) for k in range(8)], np.float32)
    assert (flips != powers).any()
    lsf = bc.LSF_PRODUCT
    flips = np.array([bc.flip_point(oracle, lsf, k) for k in range(8)], np.float32)
    above = np.array([bc.step(x, 1) for x in flips], np.float32)
    assert bc.predicted_level(oracle, flips, lsf).tolist() == list(range(8))
    assert bc.predicted_level(oracle, above, lsf).tolist() == list(range(1, 9))
    assert flips[0] == 1.0
    assert np.array_equal(flips, powers)
    # the oracle's isInFrustum agrees with the bisection's arithmetic, clamp included
    P, N, maxd, mind = bc.logf_points(np.concatenate([flips, above]), np.zeros(16, np.int64))
    r = oracle.is_in_frustum(bc.frustum(), P, N, maxd, mind)
    assert r["track_in_view"].all() and r["level"].tolist() == list(range(8)) + list(range(1, 8)) + [7]


def test_logf_case_set_has_the_sizes_it_claims(oracle, logf_set):
    c, _ = logf_set
    fam = c["family"]
    n = {k: int((fam == k).sum()) for k in np.unique(fam)}
    assert 2000 < n["flip"] < 3500 and 350_000 < n["sweep"] < 370_000 and 90_000 < n["large"] < 120_000 and n["special"] == 5 and n["tiny"] > 300
    assert len(fam) < 1_000_000
    r = c["ratio"]
    assert r.min() > np.float32(5.0) / np.float32(6.0) and np.isinf(r.max()) and (r == 1.0).any()
    assert set(np.unique(c["kexp"][fam == "sweep"])) == set(bc.DEPTH_EXPONENTS) and (c["kexp"][fam == "tiny"] == -74).all()


def test_logf_readout_is_valid_for_every_case(oracle, logf_set):
    """With log_scale_factor = the ulp of the logarithm's binade and 2^25 levels the oracle's level IS logf / ulp, and every point
    is in view: the device's level then shows every bit of the device's logf."""
    c, (P, N, maxd, mind) = logf_set
    groups = bc.readout_groups(oracle, c["ratio"])
    assert 40 < len(groups) < 80
    seen = np.zeros(len(c["ratio"]), bool)
    L = oracle.logf_n(c["ratio"])
    for lsf, idx, want in groups:
        r = oracle.is_in_frustum(bc.frustum(lsf, bc.READOUT_LEVELS), P[idx], N[idx], maxd[idx], mind[idx])
        assert r["track_in_view"].all(), lsf
        assert np.array_equal(r["level"], want), lsf
        plain = np.isfinite(L[idx]) & (L[idx] != 0)
        assert np.array_equal((want * abs(lsf))[plain], np.abs(L[idx]).astype(np.float64)[plain])      # the level gives logf back, bit for bit
        assert (want[plain] >= 1 << 23).all() and (want < 1 << 24).all()                                  # ... all 24 bits of it
        seen[idx] = True
    assert seen.all()


def test_logf_cases_with_the_product_scale(oracle, logf_set):
    c, (P, N, maxd, mind) = logf_set
    r = oracle.is_in_frustum(bc.frustum(), P, N, maxd, mind)
    assert r["track_in_view"].all()
    assert np.array_equal(np.unique(r["level"]), np.arange(8))
    assert (r["level"][c["family"] == "flip"] < 7).sum() > 500


def test_sincos_angles_cover_every_branch(oracle):
    ang = bc.sincos_angles(oracle)
    assert 4_300_000 < len(ang) < 4_600_000 and ang.min() == 0 and ang.max() == bc.step(360.0, 16) and not np.signbit(ang).any()
    r = ang * bc.FACTOR_PI
    top = (r.view(np.uint32) >> 20) & 0x7FF
    assert (top < 0x398).sum() > 30 and ((top >= 0x398) & (top < 0x3F4)).sum() > 1000          # sin = y, cos = 1 / no reduction
    n = ((np.float64(r[top >= 0x3F4]) * float.fromhex("0x1.45F306DC9C883p+23")).astype(np.int32) + 0x800000) >> 24
    assert set(np.unique(n)) == {0, 1, 2, 3, 4}                                                   # reduce_fast: every quadrant
    assert (ang == np.float32(1e-45)).any() and all((ang == np.float32(45.0 * k)).any() for k in range(9))
    # the array form of the oracle is the scalar form
    a, b = oracle.cos_sin_n(ang)
    for i in np.linspace(0, len(ang) - 1, 200).astype(int):
        assert (float(a[i]), float(b[i])) == oracle.cos_sin(ang[i])
    assert len(np.unique(a)) > 100_000 and len(np.unique(b)) > 100_000


@pytest.mark.parametrize("scene", bc.scenes(), ids=lambda s: s.name)
def test_frustum_families_sit_on_their_boundaries(oracle, scene):
    tab, names, centre = bc.frustum_scene_cases(scene)
    r = oracle.is_in_frustum(scene.frustum(), tab["pos_w"], tab["normal"], tab["max_distance"], tab["min_distance"])
    for name in np.unique(names):
        idx = np.nonzero(names == name)[0]
        c = idx[centre[idx]]
        assert len(c) == 1, name
        outs = [bc.outcome(r, i) for i in idx]
        # (PcZ = -0 against +0 has no flank: `PcZ < 0` is false for both, and 0 / -0 is the NaN that 0 / +0 is)
        assert scene.raw or any(o != bc.outcome(r, c[0]) for o in outs), f"{scene.name}/{name}: every row has the centre's outcome {outs[0]}"
    if scene.raw:
        assert r["track_in_view"].all() and np.isnan(r["proj_x"]).all() and np.isnan(r["proj_xr"]).all() and (r["track_depth"] == 0).all()
        return
    for name, kept in (("u_max", 512.0), ("u_min", 0.0)):
        c = np.nonzero((names == name) & centre)[0][0]
        assert r["track_in_view"][c] == 1 and r["proj_x"][c] == kept               # equality with a bound is kept
    for name, kept in (("v_max", 512.0), ("v_min", 0.0)):
        c = np.nonzero((names == name) & centre)[0][0]
        assert r["track_in_view"][c] == 1 and r["proj_y"][c] == kept
    for name in ("dist_min", "dist_max_6_exact", "view_cos_2^0", "view_cos_2^3"):
        assert r["track_in_view"][np.nonzero((names == name) & centre)[0][0]] == 1, name
    exact = [n for n in np.unique(names) if n.startswith("dist_max_") and n.endswith("_exact")]
    assert len(exact) >= 3
    for name in exact:
        c = np.nonzero((names == name) & centre)[0][0]
        d = np.float32(name.split("_")[2])
        assert np.float32(1.2) * tab["max_distance"][c] == d and r["track_in_view"][c] == 1      # dist == 1.2f * max_d is kept
    z0 = np.nonzero((names == "z_zero") & centre)[0][0]
    assert r["track_in_view"][z0] == 1 and np.isnan(r["proj_x"][z0])               # P = Ow: in view with NaN projections
    lv = r["level"][(names == "level_clamp") & (r["track_in_view"] == 1)]
    assert lv.min() == 0 and lv.max() == bc.NLEVELS - 1 and len(np.unique(lv)) == bc.NLEVELS
    for k in bc.FRUSTUM_KEYS:
        v = r[k][~np.isnan(r[k])] if r[k].dtype.kind == "f" else r[k]
        assert len(np.unique(v)) >= 2, k


def _oracle_local_points(oracle, v):
    import track_cases as tc
    rf = oracle.OracleFrame(v["kps"], v["desc"], None, bc.CAM["bounds"], bc.SCALE)
    fm = v["frame_mp"].copy()
    nm, r, visit = tc.oracle_local_points(oracle, rf, bc.frustum(), v["mp"], fm, v["th"], v["far"], v["th_far"])
    return nm, fm


def test_local_points_variants_differ_in_their_matches(oracle):
    by_case = {}
    for v in bc.local_points_variants():
        nm, fm = _oracle_local_points(oracle, v)
        by_case.setdefault(v["case"], {})[v["variant"]] = (nm, tuple(fm.tolist()))
    o = by_case["view_cos_0.998"]
    assert o["below"][0] == 1 and o["float_0.998"][0] == 0 and o["above"][0] == 0       # radius 4 below the double 0.998, 2.5 above
    o = by_case["th_one"]
    assert len({o["below"], o["one"], o["above"]}) == 3 and o["below"][0] == 0          # nothing, the nearer keypoint, the exact copy
    o = by_case["th_far"]
    assert o["equal"][0] == 1 and o["below"][0] == 0 and o["below_but_off"][0] == 1
    o = by_case["flags"]
    assert [o[k][0] for k in ("plain", "not_visited", "bad", "occupied", "occupied_sparsified")] == [1, 0, 0, 0, 1]
    assert o["occupied"][1] == (0,) and o["occupied_sparsified"][1] == (1,)
    nm, fm = by_case["level_band"]["all"]
    assert fm == (0, -1, 2, -1, -1, 5, 6, -1)                                          # level 0 takes octave 0 only: [-1, 0]


def _oracle_last_frame(oracle, c):
    mm = oracle.MotionModel()
    mm.q[:] = c["q"]
    mm.t[:] = c["t"]
    mm.fx, mm.fy, mm.cx, mm.cy, mm.mbf = bc.CAM["fx"], bc.CAM["fy"], bc.CAM["cx"], bc.CAM["cy"], bc.CAM["mbf"]
    mm.forward, mm.backward = int(c["forward"]), int(c["backward"])
    last = c["last"]
    valid, u, v, ur = oracle.project_last_frame(mm, bc.CAM["bounds"], last["has_point"], last["pos_w"])
    rf = oracle.OracleFrame(c["kps"], c["desc"], None, bc.CAM["bounds"], bc.SCALE)
    cur = np.full(len(c["kps"]), -1, np.int32)
    tab = dict(valid=valid, u=u, v=v, ur=ur, octave=last["octave"], angle=last["angle"], desc=last["desc"],
               mp=np.arange(len(valid), dtype=np.int32), obs=last["obs"])
    nm = rf.SearchByProjection_frames(tab, cur, c["th"], c["forward"], c["backward"], True)
    return dict(valid=valid, u=u, v=v, ur=ur), nm, cur


def test_last_frame_calls_sit_on_their_boundaries(oracle):
    zero_valid = {}
    bands = {}
    sizes = []
    for c in bc.last_frame_calls():
        proj, nm, cur = _oracle_last_frame(oracle, c)
        if c["case"] == "edges":
            names, centre = c["names"], c["centre"]
            for name in np.unique(names):
                idx = np.nonzero(names == name)[0]
                ci = idx[centre[idx]][0]
                assert len(np.unique(proj["valid"][idx])) == 2, (c["variant"], name)
                if name in ("u_max", "u_min", "v_max", "v_min"):
                    assert proj["valid"][ci] == 1 and (proj["u"][ci] in (0.0, 512.0) or proj["v"][ci] in (0.0, 512.0))
            if c["variant"] != "translated":
                z = np.nonzero(names == "z_zero")[0]
                P = c["last"]["pos_w"][z]
                neg = np.signbit(P[:, 2]) & (P[:, 2] != 0)
                assert (proj["valid"][z][neg] == 0).all()                           # invzc = -inf for the tiniest negative depth
                assert proj["valid"][z][(P[:, 2] > 0) & (P[:, 0] == 0) & (P[:, 1] == 0)].all() and np.isneginf(proj["ur"][z]).any()
            for k in ("u", "v", "ur"):
                assert len(np.unique(proj[k][~np.isnan(proj[k])])) > 2, k
        elif c["case"] == "z_signed_zero":
            zero_valid[c["variant"]] = proj["valid"].tolist()
        elif c["case"] == "level_band":
            bands[c["variant"]] = tuple(cur.tolist())
        else:
            sizes.append(len(proj["valid"]))
    # zc = +0 is kept (NaN projections), zc = -0 is rejected (invzc = -inf < 0): reached by one sign pattern of one call
    assert zero_valid["w_plus_one"] == [1] * 8 and zero_valid["w_minus_one"] == [1, 1, 1, 1, 1, 1, 0, 1]
    assert sizes == [1, 63, 64, 65, 1025]
    # point octaves (0, 0, 0, 0, 7, 7, 7, 7) against keypoint octaves (0, 1, 6, 7) twice
    assert bands["neither"] == (0, 1, -1, -1, -1, -1, 6, 7)
    assert bands["forward"] == (0, 1, 2, 3, -1, -1, -1, 7)
    assert bands["backward"] == (0, -1, -1, -1, 4, 5, 6, 7)
