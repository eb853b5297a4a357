"""msorb_sim3_ransac_batch on the CPU, before any GPU run: the restatements of tests/sim3_cases.py against each other, the scenes
held to the conditions their names promise, and ms-slam_amd/csrc/sim3_select.h / sim3_device.h compiled for the host
(tests/sim3_select_main.cc, plain and under the address / undefined-behaviour sanitizers).

R32 is the float32 statement the device must reproduce bit for bit; R64 is the reference's path (float64, numpy.linalg.eigh,
atan2, Rodrigues).  Measured and recorded in tests/golden/sim3_ransac_sensitivity.json: the two return the same winner, converged
flag, consumed count and winner's mask on every scene, and differ in 1 of 484 892 (hypothesis, correspondence) decisions; the
winner's R differs by at most 1.2e-5, t by 6.6e-5 of its largest component, s by 1.5e-7 (the largest figures belong to a winner
drawn from a nearly collinear triple).  That distance is what float rounding gives, and is the unit any bound on the device
would be stated in; the GPU test needs none, because the device equals R32 bit for bit."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import sim3_cases as s3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name, mk in s3.SCENES.items():
        sc = mk()
        out[name] = (sc, s3.R32(sc, detail=True), s3.R64(sc, detail=True))
    return out


def test_scene_list_covers_what_it_names(runs):
    n_of = {name: len(sc["X1"]) for name, (sc, _, _) in runs.items()}
    assert {3, 63, 64, 65, 255, 256, 257, 1025} <= set(n_of.values())
    h_of = {len(sc["triples"]) for sc, _, _ in runs.values()}
    assert 1 in h_of and 300 in h_of
    assert {sc["fix_scale"] for sc, _, _ in runs.values()} == {True, False}
    sc, r, _ = runs["min_inliers=n"]
    assert sc["min_inliers"] == len(sc["X1"]) and s3.ransac_max_its(0.99, sc["min_inliers"], len(sc["X1"]), 300) == 1 == len(sc["triples"])
    assert any(r["converged"] and 0 < r["winner"] for _, r, _ in runs.values())           # a converged run, not at the first draw
    sc, r, _ = runs["exhausted"]
    assert not r["converged"] and r["consumed"] == len(sc["triples"]) == 300 and r["winner"] >= 0
    sc, r, _ = runs["ties"]                                                              # `>=` and not `>` replaces
    first = int(np.nonzero(r["counts"] >= sc["best_inliers_in"])[0][0])
    assert not r["converged"] and r["winner"] > first and r["counts"][first] == r["counts"][r["winner"]]
    strict, best = -1, sc["best_inliers_in"] - 1
    for i, c in enumerate(r["counts"]):
        if c > best:
            strict, best = i, c
    assert strict != r["winner"]
    sc, r, _ = runs["best_in_reached"]
    assert sc["best_inliers_in"] > 0 and r["winner"] >= 0 and (r["counts"][:r["winner"]] < sc["best_inliers_in"]).any()
    assert r["winner"] != s3.select(r["counts"], sc["min_inliers"], 0)[0] or (r["counts"] < sc["best_inliers_in"]).any()
    sc, r, _ = runs["best_in_unreached"]
    assert r["winner"] == -1 and r["consumed"] == len(sc["triples"]) and not r["inliers"].any() and r["n_inliers"] == 0
    sc, r, _ = runs["coincident_free"]                                                   # NaN scale, no inlier, still in the scan
    assert np.isnan(r["T"]["s"][0]) and r["counts"][0] == 0
    sc, r, _ = runs["coincident_fixed"]
    assert np.array_equal(r["T"]["R"][0], np.eye(3, dtype=np.float32)) and r["T"]["s"][0] == 1
    sc, r, _ = runs["behind"]
    w = r["winner"]
    z = r["T"]["sR"][w, 2] @ sc["X2"][5] + r["T"]["t"][w, 2]
    assert w >= 0 and z <= 0 and sc["X1"][6, 2] == 0 and not np.isfinite(r["err1"][w, 6]) and not r["mask"][:, 6].any()
    assert len({(len(runs[k][0]["X1"]), len(runs[k][0]["triples"])) for k in s3.BATCH}) == 3


def test_r32_and_r64_agree_as_recorded(runs):
    rec = json.load(open(s3.FIXTURE))
    assert set(rec) == set(s3.SCENES)
    for name, (sc, a, b) in runs.items():
        m = s3.measure(sc)
        print(name, m)
        assert m["agree"], name                                   # winner, converged, consumed, the winner's mask
        assert m["share_differing"] <= 1e-3, (name, m)
        r = rec[name]
        assert m["decisions"] == r["decisions"] and m["decisions_differing"] <= r["decisions_differing"], (name, m)
        for k in ("R_abs", "t_rel", "s_rel"):
            assert (m.get(k) is None) == (r[k] is None) and (r[k] is None or m[k] <= r[k]), (name, k, m)
        k = "winner_closest_to_threshold"
        assert (m.get(k) is None) == (r[k] is None) and (r[k] is None or m[k] >= r[k]), (name, m)


def test_select_is_the_literal_loop():
    assert s3.select([], 5, 0) == (-1, 0, 0, 0)
    assert s3.select([3, 3, 2], 5, 0) == (1, 0, 3, 3)           # a tie goes to the later hypothesis
    assert s3.select([3, 6, 9], 5, 0) == (1, 1, 2, 6)           # stops at the first count > min_inliers that is >= best
    assert s3.select([3, 6, 9], 5, 7) == (2, 1, 3, 9)           # 6 > min_inliers but below the carried best
    assert s3.select([3, 4], 5, 7) == (-1, 0, 2, 7)
    assert s3.select([5, 5], 5, 0) == (1, 0, 2, 5)              # count == min_inliers does not converge


@pytest.fixture(scope="module")
def mains(tmp_path_factory):
    d = tmp_path_factory.mktemp("sim3_select_main")
    src = os.path.join(ROOT, "tests", "sim3_select_main.cc")
    flags = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", f"-I{ROOT}/ms-slam_amd/csrc"]
    exes = {}
    for tag, extra in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[tag] = str(d / tag)
        b = subprocess.run(["g++", *flags, *extra, src, "-o", exes[tag]], capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr
    return d, exes


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_select_header_on_the_host(mains, build):
    """random count vectors with many ties, empty ranges, carried bests above, inside and below the counts"""
    d, exes = mains
    rng = np.random.RandomState(5)
    cases = [([], 3, 0), ([], 3, 9), ([4], 3, 4), ([4], 4, 4), ([4], 3, 5)]
    for _ in range(400):
        n = int(rng.choice([0, 1, 2, 7, 8, 63, 64, 65, 300]))
        hi = int(rng.choice([2, 5, 40]))
        cases.append((rng.randint(0, hi + 1, n).tolist(), int(rng.randint(0, hi + 2)), int(rng.randint(0, hi + 3))))
    fin = str(d / f"select_{build}.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for counts, mn, best in cases:
            f.write(struct.pack("<3i", len(counts), mn, best) + np.asarray(counts, np.int32).tobytes())
    p = subprocess.run([exes[build], "select", fin], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-400:], p.stderr[-2000:])
    got = [tuple(int(x) for x in line.split()) for line in p.stdout.splitlines()]
    assert got == [s3.select(c, mn, best) for c, mn, best in cases]
    assert sum(g[1] for g in got) > 50 and sum(g[0] == -1 for g in got) > 20


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_device_header_on_the_host_equals_r32_bit_for_bit(runs, mains, build):
    d, exes = mains
    for name, (sc, r, _) in runs.items():
        n, H = len(sc["X1"]), len(sc["triples"])
        fin, fout = str(d / "eval_in.bin"), str(d / "eval_out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<3i", n, H, int(sc["fix_scale"])) + sc["cam1"].tobytes() + sc["cam2"].tobytes() + sc["X1"].tobytes() +
                    sc["X2"].tobytes() + sc["max_err1"].tobytes() + sc["max_err2"].tobytes() + sc["triples"].tobytes())
        p = subprocess.run([exes[build], "eval", fin, fout], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (name, p.stderr[-2000:])
        raw = open(fout, "rb").read()
        assert len(raw) == 4 * H + 52 * H + H * n
        counts = np.frombuffer(raw, np.int32, H)
        rec = np.frombuffer(raw, np.uint32, 13 * H, 4 * H).reshape(H, 13)
        mask = np.frombuffer(raw, np.uint8, H * n, 56 * H).reshape(H, n).astype(bool)
        assert np.array_equal(counts, r["counts"]) and np.array_equal(mask, r["mask"]), name
        want = np.concatenate([r["T"]["s"][:, None], r["T"]["R"].reshape(H, 9), r["T"]["t"]], 1).astype(np.float32)
        fin_ = np.isfinite(want)
        assert np.array_equal(np.isfinite(rec.view(np.float32)), fin_), name
        assert np.array_equal(rec[fin_], want.view(np.uint32)[fin_]), name


def test_bad_arguments_are_refused_before_a_device_is_touched(msorb_mod):
    """every refusal of msorb_sim3_ransac_batch is decided before the device is looked for, so it is the same with or without one;
    the outputs stay as they were"""
    sc = s3.SCENES["H=1"]()
    n = len(sc["X1"])
    E = msorb_mod.E_INVALID

    def call(**kw):
        return s3.raw_call(msorb_mod, sc, **kw)

    assert call(n_problems=-1) == (E, True)
    assert call(n=2, triples=[[0, 1, 0]]) == (E, True)                          # n < 3
    assert call(n_hyp=0, hyp=(0, 0)) == (E, True)                               # H < 1
    assert call(triples=[[4, 9, 4]]) == (E, True)                               # a repeated index
    assert call(triples=[[0, 1, n]]) == (E, True)                               # an index >= n
    assert call(triples=[[0, -1, 2]]) == (E, True)
    assert call(corr=(0, n - 1)) == (E, True) and call(hyp=(1, 2)) == (E, True)  # offsets that do not match
    for k in ("problems", "corr", "hyp", "X1", "X2", "e1", "e2", "triples", "inl", "res"):
        assert call(null=(k,)) == (E, True), k
    assert call(n_problems=0) == (msorb_mod.OK, True)
