"""The comparisons of frustum_point (frustum_kernel and the fused local_points_kernel) and of last_frame_point ON their
boundaries: inputs built from exactly representable numbers so that u == max_x, dist == 1.2f * max_d, viewCos == the limit,
(double)viewCos > 0.998, depth == thFarPoints, a depth of +0 / -0 / the smallest subnormal, non-finite inputs and the level
clamps are hit, each with its neighbours (tests/boundary_cases.py; tests/test_boundary_cases_cpu.py holds the sets to that).
Everything against the oracle, bit for bit; a NaN equals any NaN."""
import numpy as np
import pytest

import boundary_cases as bc
import track_cases as tc

pytestmark = pytest.mark.gpu


def _assert_same(a, b, keys, what):
    for k in keys:
        if not bc.same_bits(a[k], b[k]):
            bad = np.nonzero(~((a[k] == b[k]) | (np.isnan(a[k].astype(np.float64)) & np.isnan(b[k].astype(np.float64)))))[0][:8]
            raise AssertionError(f"{what}: {k} differs at rows {bad.tolist()}: device {a[k][bad].tolist()} oracle {b[k][bad].tolist()}")


@pytest.mark.parametrize("scene", bc.scenes(), ids=lambda s: s.name)
def test_frustum_point_on_its_boundaries(msorb_mod, oracle, scene):
    tab, names, _ = bc.frustum_scene_cases(scene)
    F = scene.frustum()
    b = oracle.is_in_frustum(F, tab["pos_w"], tab["normal"], tab["max_distance"], tab["min_distance"])
    a = msorb_mod.is_in_frustum(F, tab["pos_w"], tab["normal"], tab["max_distance"], tab["min_distance"])
    print(f"{scene.name}: {len(names)} rows in {len(np.unique(names))} families, {int(b['track_in_view'].sum())} in view")
    for name in np.unique(names):
        sel = names == name
        _assert_same({k: a[k][sel] for k in bc.FRUSTUM_KEYS}, {k: b[k][sel] for k in bc.FRUSTUM_KEYS}, bc.FRUSTUM_KEYS, f"frustum_kernel {scene.name}/{name}")
    # the same rows through the fused kernel, on a frame of one keypoint
    kps, kdesc = bc.minimal_frame()
    f = msorb_mod.Frame(kps, kdesc, None, bc.CAM["bounds"], bc.SCALE)
    rf = oracle.OracleFrame(kps, kdesc, None, bc.CAM["bounds"], bc.SCALE)
    try:
        fa, fb = np.full(1, -1, np.int32), np.full(1, -1, np.int32)
        nm, out = msorb_mod.search_local_points(f, F, tab, fa, 1.0)
        rnm, r, _ = tc.oracle_local_points(oracle, rf, F, tab, fb, 1.0)
        _assert_same(out, r, bc.FRUSTUM_KEYS, f"local_points_kernel {scene.name}")
        assert nm == rnm and np.array_equal(fa, fb)
    finally:
        f.close()


VARIANTS = bc.local_points_variants()


@pytest.mark.parametrize("v", VARIANTS, ids=[f"{v['case']}-{v['variant']}" for v in VARIANTS])
def test_local_points_kernel_decisions(msorb_mod, oracle, v):
    """RadiusByViewingCos at 0.998, th == 1.0f, depth == thFarPoints, the flags, the level band: seen through the matches"""
    F = bc.frustum()
    f = msorb_mod.Frame(v["kps"], v["desc"], None, bc.CAM["bounds"], bc.SCALE)
    rf = oracle.OracleFrame(v["kps"], v["desc"], None, bc.CAM["bounds"], bc.SCALE)
    try:
        fa, fb = v["frame_mp"].copy(), v["frame_mp"].copy()
        nm, out = msorb_mod.search_local_points(f, F, v["mp"], fa, v["th"], v["far"], v["th_far"])
        rnm, r, visit = tc.oracle_local_points(oracle, rf, F, v["mp"], fb, v["th"], v["far"], v["th_far"])
        print(f"{v['case']}/{v['variant']}: oracle {rnm} matches {fb.tolist()}, device {nm} matches {fa.tolist()}")
        assert nm == rnm and np.array_equal(fa, fb)
        assert np.array_equal(out["track_in_view"].astype(bool), r["track_in_view"].astype(bool) & visit)
        _assert_same({k: out[k][visit] for k in bc.FRUSTUM_KEYS}, {k: r[k][visit] for k in bc.FRUSTUM_KEYS}, bc.FRUSTUM_KEYS, v["variant"])
    finally:
        f.close()


CALLS = bc.last_frame_calls()


@pytest.mark.parametrize("c", CALLS, ids=[f"{c['case']}-{c['variant']}" for c in CALLS])
def test_last_frame_point_on_its_boundaries(msorb_mod, oracle, c):
    def model(mod):
        return mod.MotionModel.make(c["q"], c["t"], bc.CAM["fx"], bc.CAM["fy"], bc.CAM["cx"], bc.CAM["cy"], bc.CAM["mbf"], c["forward"], c["backward"])
    last = c["last"]
    f = msorb_mod.Frame(c["kps"], c["desc"], None, bc.CAM["bounds"], bc.SCALE)
    rf = oracle.OracleFrame(c["kps"], c["desc"], None, bc.CAM["bounds"], bc.SCALE)
    try:
        msorb_mod.frame_set_last_points(f, last)
        cur, want = np.full(len(c["kps"]), -1, np.int32), np.full(len(c["kps"]), -1, np.int32)
        nm, proj = msorb_mod.search_last_frame(f, model(msorb_mod), last["obs"], cur, c["th"], True, want_projection=True)
        omm = oracle.MotionModel()
        omm.q[:] = c["q"]
        omm.t[:] = c["t"]
        omm.fx, omm.fy, omm.cx, omm.cy, omm.mbf = bc.CAM["fx"], bc.CAM["fy"], bc.CAM["cx"], bc.CAM["cy"], bc.CAM["mbf"]
        omm.forward, omm.backward = int(c["forward"]), int(c["backward"])
        valid, u, vv, ur = oracle.project_last_frame(omm, bc.CAM["bounds"], last["has_point"], last["pos_w"])
        wproj = dict(valid=valid, u=u, v=vv, ur=ur)
        tab = dict(valid=valid, u=u, v=vv, ur=ur, octave=last["octave"], angle=last["angle"], desc=last["desc"],
                   mp=np.arange(len(valid), dtype=np.int32), obs=last["obs"])
        wnm = rf.SearchByProjection_frames(tab, want, c["th"], c["forward"], c["backward"], True)
        print(f"{c['case']}/{c['variant']}: {len(valid)} points, {int(valid.sum())} valid, oracle {wnm} matches, device {nm}")
        _assert_same(proj, wproj, ("valid", "u", "v", "ur"), f"last_frame_point {c['case']}/{c['variant']}")
        assert nm == wnm and np.array_equal(cur, want)
    finally:
        f.close()


@pytest.fixture(scope="module")
def square_frame(msorb_mod):
    """a 512 x 512 stereo pair (the image bounds of boundary_cases.CAM) and its extraction"""
    from msorb import synth
    L, R = synth.stereo_pair(5, 512, 512)
    ex = msorb_mod.ORBextractor(500, 1.2, bc.NLEVELS, 20, 7)
    mbf = bc.CAM["mbf"]
    mb = mbf / bc.CAM["fx"]
    kl, dl, kr, dr, ur, dp, oob = ex.extract_stereo(L, R, mb, mbf)
    yield dict(L=L, R=R, ex=ex, mb=mb, mbf=mbf, kl=kl, dl=dl, ur=ur, scale=ex.GetScaleFactors())
    ex.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_last_frame_point_in_the_tail_blocks_of_the_grid_launch(msorb_mod, oracle, square_frame, n):
    """msorb_track_frontend_motion projects the last frame's points in the blocks BEHIND the grid blocks of frame_grid_kernel (1024
    threads each): a partial block, and a full one with a partial one.  The table alternates the boundary rows with points on the
    viewing rays of the frame's own keypoints, so the projection is seen through matches."""
    s = square_frame
    P, names, _ = bc.last_frame_edge_rows()
    kl, dl = s["kl"], s["dl"]
    assert len(kl) > 200
    pos = np.zeros((n, 3), np.float32)
    desc = np.zeros((n, 32), np.uint8)
    octv = np.zeros(n, np.int32)
    for i in range(n):
        if i % 2:
            pos[i] = P[(i // 2) % len(P)]
            desc[i] = bc.descriptor(3)
        else:
            k = (i // 2 * 7) % len(kl)
            pos[i] = ((kl["x"][k] - 256.0) * 4.0 / 512.0, (kl["y"][k] - 256.0) * 4.0 / 512.0, 4.0)
            desc[i] = dl[k]
            octv[i] = kl["octave"][k]
    last = dict(has_point=np.ones(n, np.uint8), pos_w=pos, octave=octv, angle=np.zeros(n, np.float32), desc=desc, obs=np.ones(n, np.int32))
    ident, zero = (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0)
    mm = msorb_mod.MotionModel.make(ident, zero, bc.CAM["fx"], bc.CAM["fy"], bc.CAM["cx"], bc.CAM["cy"], s["mbf"])
    f, st, cur, nm = msorb_mod.track_frontend_motion(s["ex"], s["L"], s["R"], s["mb"], s["mbf"], mm, last, last["obs"], 7.0, check_orientation=False)
    try:
        assert np.array_equal(st[0].view(np.uint8), kl.view(np.uint8))
        omm = oracle.MotionModel()
        omm.q[:] = ident
        omm.t[:] = zero
        omm.fx, omm.fy, omm.cx, omm.cy, omm.mbf = bc.CAM["fx"], bc.CAM["fy"], bc.CAM["cx"], bc.CAM["cy"], s["mbf"]
        valid, u, v, ur = oracle.project_last_frame(omm, bc.CAM["bounds"], last["has_point"], pos)
        rf = oracle.OracleFrame(kl, dl, s["ur"], bc.CAM["bounds"], s["scale"])
        want = np.full(len(kl), -1, np.int32)
        tab = dict(valid=valid, u=u, v=v, ur=ur, octave=octv, angle=last["angle"], desc=desc, mp=np.arange(n, dtype=np.int32), obs=last["obs"])
        wnm = rf.SearchByProjection_frames(tab, want, 7.0, False, False, False)
        print(f"table of {n}: {int(valid.sum())} valid, oracle {wnm} matches, device {nm}")
        assert wnm >= (n + 1) // 2 * 0.5          # most of the points on keypoint rays find their keypoint
        assert nm == wnm and np.array_equal(cur, want)
        # and the projection of the table the handle now holds, by the kernel of its own
        cur2 = np.full(len(kl), -1, np.int32)
        _, proj = msorb_mod.search_last_frame(f, mm, last["obs"], cur2, 7.0, False, want_projection=True)
        _assert_same(proj, dict(valid=valid, u=u, v=v, ur=ur), ("valid", "u", "v", "ur"), f"table of {n}")
    finally:
        f.close()
