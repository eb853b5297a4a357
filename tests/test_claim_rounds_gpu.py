"""Device rounds of the claim-replaying searches are behaviour: a replay that asks for a new round more often than it must still
gives the reference's matches, so the oracle comparisons cannot see it.  Small dense scenes — about 300 keypoints inside a 3x3-cell
region of the 64x48 grid, several queries per keypoint, so that candidate lists of kTopK are exhausted by earlier claims and points
without observations free occupied keypoints — through msorb_search_by_projection_mps, msorb_search_by_projection_frames and
msorb_search_by_projection_mps_rig: the result equals the oracle's and msorb_frame_search_rounds (per camera for the rig) equals
tests/golden/claim_rounds.json.  That file was recorded with the library of the commit it names, BEFORE the replay was made one
component (`python tests/test_claim_rounds_gpu.py out.json` with MSORB_LIB pointing at that build re-records it); every recorded
scene needed at least 2 rounds there."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "claim_rounds.json")
SCALE = np.array([1.2 ** i for i in range(8)], np.float32)
BOUNDS = (0.0, 1241.0, 0.0, 376.0)
CELL_W, CELL_H = 1241.0 / 64, 376.0 / 48

with open(GOLDEN) as _f:
    RECORD = json.load(_f)


def dense_camera(rng, oracle, n):
    """n keypoints inside grid cells [20, 23) x [20, 23), octaves 0..3"""
    k = np.zeros(n, oracle.KP_DTYPE)
    k["x"] = rng.uniform(20 * CELL_W + 0.01, 23 * CELL_W - 0.01, n)
    k["y"] = rng.uniform(20 * CELL_H + 0.01, 23 * CELL_H - 0.01, n)
    k["octave"] = rng.integers(0, 4, n); k["angle"] = rng.uniform(0, 360, n); k["size"] = 31
    return k, rng.integers(0, 256, (n, 32), dtype=np.uint8)


def run_scene(msorb_mod, oracle, sc):
    """-> (result equals the oracle's, [rounds of the last search per frame])"""
    import matcher_cases as mc
    rng = np.random.Generator(np.random.PCG64(sc["seed"]))
    n, M, th = sc["n_keypoints"], sc["n_queries"], sc["th"]
    no_ur = np.full(n, -1, np.float32)
    k, d = dense_camera(rng, oracle, n)
    if sc["entry"] == "mps_rig":
        k2, d2 = dense_camera(rng, oracle, n)
        l2r, r2l = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        li, ri = rng.permutation(n)[:n * 6 // 10], rng.permutation(n)[:n * 6 // 10]
        l2r[li] = ri; r2l[ri] = li
        d2[ri] = mc.flip_bits(rng, d[li], 25); k2["octave"][ri] = k["octave"][li]
        mp = mc.map_point_table(rng, k, d, no_ur, SCALE, M, 0.15, 0.05)
        src = rng.integers(0, n, M)            # the right camera's projections: near some right keypoint, at its level or the next
        mp.update(track_in_view_r=(rng.random(M) < 0.9).astype(np.uint8), proj_xr=(k2["x"][src] + rng.normal(0, 3, M)).astype(np.float32),
                  proj_yr=(k2["y"][src] + rng.normal(0, 3, M)).astype(np.float32),
                  level_r=(k2["octave"][src] + rng.integers(0, 2, M)).astype(np.int32), view_cos_r=rng.uniform(0.99, 1.0, M).astype(np.float32))
        init = np.where(rng.random(2 * n) < 0.2, rng.integers(0, M, 2 * n), -1).astype(np.int32)
        frames = [msorb_mod.Frame(k, d, None, BOUNDS, SCALE), msorb_mod.Frame(k2, d2, None, BOUNDS, SCALE)]
        refs = [oracle.OracleFrame(k, d, None, BOUNDS, SCALE), oracle.OracleFrame(k2, d2, None, BOUNDS, SCALE)]
        got, want = init.copy(), init.copy()
        gn = msorb_mod.search_by_projection_mps_rig(frames[0], frames[1], mp, l2r, r2l, got, th, False, 50.0, 0.8)
        wn = oracle.search_by_projection_mps_rig(refs[0], refs[1], mp, l2r, r2l, want, th, False, 50.0, 0.8)
    else:
        frames, rf = [msorb_mod.Frame(k, d, None, BOUNDS, SCALE)], oracle.OracleFrame(k, d, None, BOUNDS, SCALE)
        if sc["entry"] == "mps":
            mp = mc.map_point_table(rng, k, d, no_ur, SCALE, M, 0.15, 0.05)
            init = np.where(rng.random(n) < 0.2, rng.integers(0, M, n), -1).astype(np.int32)
            got, want = init.copy(), init.copy()
            gn = frames[0].SearchByProjection_mps(mp, got, th, False, 50.0, 0.8)
            wn = rf.SearchByProjection_mps(mp, want, th, False, 50.0, 0.8)
        else:
            assert sc["entry"] == "frames"
            last = mc.last_frame_table(rng, k, d, no_ur, SCALE, M)
            init = np.where(rng.random(n) < 0.2, rng.integers(0, M, n), -1).astype(np.int32)
            got, want = init.copy(), init.copy()
            gn = frames[0].SearchByProjection_frames(last, got, th)
            wn = rf.SearchByProjection_frames(last, want, th)
    try:
        rounds = [int(msorb_mod.frame_search_rounds(f)[0]) for f in frames]
    finally:
        for f in frames:
            f.close()
    return bool(gn == wn and wn > n // 10 and np.array_equal(got, want)), rounds


def test_the_record_is_of_scenes_that_needed_new_rounds():
    assert len(RECORD["commit"]) >= 7
    assert {s["entry"] for s in RECORD["scenes"]} == {"mps", "frames", "mps_rig"}
    for s in RECORD["scenes"]:
        assert len(s["rounds"]) == (2 if s["entry"] == "mps_rig" else 1) and min(s["rounds"]) >= 2, s


@pytest.mark.parametrize("sc", RECORD["scenes"], ids=lambda s: f"{s['entry']}-seed{s['seed']}")
def test_result_and_rounds(msorb_mod, oracle, sc):
    same, rounds = run_scene(msorb_mod, oracle, sc)
    print(sc["entry"], sc["seed"], "rounds", rounds, "recorded", sc["rounds"])
    assert same, "the result differs from the oracle's"
    assert rounds == sc["rounds"]


if __name__ == "__main__":   # re-record: MSORB_LIB=<the parent commit's libmsorb.so> python tests/test_claim_rounds_gpu.py out.json <commit>
    ROOT = os.path.dirname(HERE)
    sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.join(ROOT, "oracle"), HERE]
    import msorb
    import orb_oracle
    msorb.lib(); orb_oracle.lib()
    out = dict(RECORD, commit=sys.argv[2])
    for s in out["scenes"]:
        same, s["rounds"] = run_scene(msorb, orb_oracle, s)
        print(s, "equals the oracle" if same else "DIFFERS from the oracle", flush=True)
        assert same
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
