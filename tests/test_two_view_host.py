"""ms-slam_amd/csrc/two_view_device.h and two_view_select.h, the text the kernels compile, built for the host as
tests/two_view_main.cc (plain at -O2, and under the address / undefined-behaviour sanitizers) and run directly, against R64 of
tests/two_view_cases.py (the reference's path in numpy float64, which shares no step with the header).

On every admitted scene the program agrees with R64 on every decision: ok, branch, both winners, the chosen motion hypothesis,
every nGood, the winner's mask and triangulated (the motion hypotheses paired by value: their order hangs on the signs an SVD hands
out).  A bit of the winner's mask may differ only where R64's chi-square is closer to the threshold than float rounding
(two_view_cases.mask_excuse); the count is printed: 0 on the 32 scenes.  R, t and p3d / depth lie within 16 times the largest
difference measured by running tests/two_view_cases.py as a script (tests/golden/two_view_spread.json: 8.3e-4, 4.1e-4, 1.3e-3; the
float64 variants among themselves spread 2.5e-4, 1.3e-4, 3.0e-4; 79 of 1 871 176 (hypothesis, match) decisions differ; the
smallest relative gap between a winner's score and the runner-up is 2.0e-4).  No GPU, nothing loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import two_view_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mains(tmp_path_factory):
    d = tmp_path_factory.mktemp("two_view_main")
    src = os.path.join(ROOT, "tests", "two_view_main.cc")
    flags = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]
    exes = {}
    for tag, extra in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[tag] = str(d / tag)
        b = subprocess.run(["g++", *flags, *extra, src, "-o", exes[tag], "-lpthread"], capture_output=True, text=True, timeout=300)
        assert b.returncode == 0, b.stderr
    return d, exes


def test_scene_list_covers_what_it_names():
    admitted = tc.admitted()
    assert set(tc.EDGE) <= set(admitted) and len(tc.GENERATED) - len([n for n in tc.GENERATED if n in admitted]) <= len(tc.GENERATED) // 10
    runs = {n: tc.prepared(n) for n in admitted}
    assert {8, 63, 64, 65, 255, 256, 257, 1025} <= {r["n"] for _, r in runs.values()}
    assert {1, 200} <= {len(sc["sets"]) for sc, _ in runs.values()}
    sc, r = runs["n=8,set=all"]
    assert sorted(sc["sets"][0]) == list(range(8)) and r["n"] == 8 and r["counts"][1, 0] == 8
    # both branches, success and every way to fail
    assert any(r["branch"] == tc.FUNDAMENTAL and r["ok"] for _, r in runs.values())
    for name in ("F fails: pure rotation", "F fails: n=65,40% outliers", "F fails: n=1025,40% outliers"):
        sc, r = runs[name]
        good = [c["n_good"] for c in r["checks"]]
        assert r["branch"] == tc.FUNDAMENTAL and not r["ok"], name
        assert (max(good) < max(int(0.9 * r["n_inliers"]), 50)) != (sum(g > 0.7 * max(good) for g in good) > 1), name   # one cause each
    assert sum(g > 0.7 * 237 for g in [c["n_good"] for c in runs["F fails: pure rotation"][1]["checks"]]) == 2
    sc, r = runs["H: plane"]
    assert r["branch"] == tc.HOMOGRAPHY and r["ok"] and sc["h_ratio"] == 0.40 and 0.40 < r["RH"] < 0.50 and len(r["checks"]) == 8
    sc, r = runs["H at 0.50,H=1"]          # the reference's constant: found with one iteration (155 of 1000 seeds), not with 200
    assert r["branch"] == tc.HOMOGRAPHY and r["ok"] and sc["h_ratio"] == 0.5 and r["RH"] > 0.5 and len(sc["sets"]) == 1
    sc, r = runs["H fails: second best"]
    good = sorted(c["n_good"] for c in r["checks"])
    assert r["branch"] == tc.HOMOGRAPHY and not r["ok"] and good[-2] >= 0.75 * good[-1] > 50
    sc, r = runs["H fails: identical images"]
    assert r["branch"] == tc.HOMOGRAPHY and not r["ok"] and r["motions"] == [] and r["n_inliers"] == 100
    # the order statistic: fewer than 51 accepted, exactly 51, more
    assert max(c["n_good"] for c in runs["accepted<51"][1]["checks"]) == 40
    assert max(c["n_good"] for c in runs["accepted==51"][1]["checks"]) == 51
    assert max(c["n_good"] for c in runs["n=1025,H=200"][1]["checks"]) > 600
    sc, r = runs["repeated pair"]
    i1, i2 = tc.matches_of(sc)
    assert np.array_equal(sc["keys1"][i1[0]], sc["keys1"][i1[1]]) and np.array_equal(sc["keys2"][i2[0]], sc["keys2"][i2[1]])
    assert {0, 1} <= set(sc["sets"][0]) and r["winner_h"] != 0 and r["winner_f"] != 0
    sc, r = runs["all outliers"]
    assert r["branch"] == tc.NO_MODEL and r["SH"] == 0 and r["SF"] == 0 and not r["ok"] and not (r["scores"] > 0).any()
    sc, r = runs["behind and far"]
    c = r["checks"][r["chosen"]]
    inl = r["inliers"]
    assert ((c["status"] == 0) & inl & (c["z1"] <= 0) & (c["cos"] < 0.99998)).any()      # behind, with parallax: rejected at :851
    assert ((c["status"] == 1) & (c["z1"] <= 0)).any()                                    # behind, without: counted, not vbGood
    assert (c["status"] == 2).sum() > 100
    for name in ("unmatched keypoints", "n=257", "n=1025,H=200"):
        sc, r = runs[name]
        i1, _ = tc.matches_of(sc)
        assert len(sc["keys1"]) > r["n"] and len(sc["keys2"]) > r["n"]
        assert abs(sc["keys1"][:, 0].mean() - sc["keys1"][i1, 0].mean()) > 5, name      # Normalize over all keypoints is another T


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_the_header_on_the_host_against_r64(mains, build):
    d, exes = mains
    names = tc.admitted()
    prep = [tc.prepared(n) for n in names]
    rec = tc.load_spread()
    bound = {k: 16 * v for k, v in rec["float_minus_r64"].items()}
    answers = tc.run_program(exes[build], [sc for sc, _ in prep], str(d), "run_" + build)
    excused = differing = 0
    for name, (sc, ref), ans in zip(names, prep, answers):
        x = tc.as_evaluation(ans)
        allow = tc.mask_excuse(sc, ref)
        dR, dt, dp = tc.result_difference(x, ref)
        bits = int((ans["inliers"] != ref["inliers"]).sum())
        hyp_bits = int((ans["masks"] != ref["masks"]).sum())
        excused += bits
        differing += hyp_bits
        print(f"{name}: R {dR:.2e} (bound {bound['R']:.2e}) t {dt:.2e} ({bound['t']:.2e}) p3d/depth {dp:.2e} ({bound['p3d_rel']:.2e}); "
              f"winner's mask bits differing {bits}, of all hypotheses {hyp_bits} of {ref['masks'].size}")
        why = tc.decisions_differ(x, ref, allow)
        assert why is None, (name, why)
        assert dR <= bound["R"] and dt <= bound["t"] and dp <= bound["p3d_rel"], (name, dR, dt, dp)
        r = ans["result"]
        # the record is consistent with the lists it was taken from
        m, ch = int(r["n_motion"]), int(r["chosen"])
        assert m == len(ref["motions"]) and (r["n_good"][m:] == 0).all()
        if ch >= 0:
            assert r["R"].tobytes() == r["motion_R"][ch].tobytes() and r["t"].tobytes() == r["motion_t"][ch].tobytes()
            i1, _ = tc.matches_of(sc)
            st = ans["status"][ch]
            assert np.array_equal(ans["triangulated"][i1], st == 2) and not ans["triangulated"].sum() > (st == 2).sum()
            assert int(r["n_good"][ch]) == int((st > 0).sum()) == int((np.abs(ans["p3d"]).sum(1) > 0).sum())
        else:
            assert not ans["triangulated"].any() and not ans["p3d"].any() and not r["R"].any() and not r["t"].any()
    print(f"winner's mask bits excused: {excused}; (hypothesis, match) decisions differing: {differing}")


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_the_selection_rule_against_a_plain_loop(mains, build):
    d, exes = mains
    rng = np.random.RandomState(11)
    cases, payload = [], [b""]
    for k in range(480):
        kind = k % 4
        if kind == 0:
            n = int(rng.randint(1, 30))
            s = rng.uniform(-5, 40, n).astype(np.float32)
            if k % 8 == 0:
                s = -np.abs(s)                               # nothing exceeds 0
            if k % 12 == 0:
                s[rng.randint(n)] = np.nan                   # a NaN never wins
            if k % 16 == 0 and n > 2:
                s[n // 2] = s[0] = np.float32(41.0)          # a tie: the first stays
            cases.append((0, s))
            payload.append(np.int32([0, n]).tobytes() + s.tobytes())
        elif kind == 1:
            SH, SF = np.float32(rng.uniform(0, 900)), np.float32(rng.uniform(0, 900))
            if k % 3 == 0:
                SH = SF = np.float32(0)
            if k % 5 == 0:
                SF = SH                                      # RH == 0.5 exactly: not above 0.50
            hr = [0.5, 0.4, 0.45][k % 3]
            cases.append((1, SH, SF, hr))
            payload.append(np.int32([1]).tobytes() + np.float32([SH, SF]).tobytes() + np.float64(hr).tobytes())
        else:
            m = 4 if kind == 2 else 8
            n_inl = int(rng.randint(8, 120))
            good = rng.randint(0, n_inl + 1, m).astype(np.int32)
            style = (k // 4) % 4
            if style == 0:
                good[:] = rng.randint(0, 5, m)
                good[rng.randint(m)] = n_inl - rng.randint(0, 3)          # a clear winner
            if style == 1:
                good[:] = 0
                a, b = rng.choice(m, 2, replace=False)
                good[a], good[b] = n_inl, int(n_inl * rng.choice([0.7, 0.72, 0.75, 0.76, 1.0]))   # at the edges of 0.7 / 0.75
            par = rng.choice([0.0, 0.5, 1.0, 1.5, 3.0], m).astype(np.float32)
            mt = int(rng.choice([5, 50]))
            cases.append((kind, good, par, n_inl, mt))
            payload.append(np.int32([kind, n_inl, mt]).tobytes() + np.float32([1.0]).tobytes() + good.tobytes() + par.tobytes())
    fin, fout = str(d / f"select_{build}.in"), str(d / f"select_{build}.out")
    with open(fin, "wb") as f:
        f.write(np.int32(len(cases)).tobytes() + b"".join(payload))
    p = subprocess.run([exes[build], "select", fin, fout], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    raw = open(fout, "rb").read()
    assert len(raw) == 8 * len(cases)
    seen = set()
    for i, c in enumerate(cases):
        a, b = raw[8 * i:8 * i + 4], raw[8 * i + 4:8 * i + 8]
        if c[0] == 0:
            score, winner = tc.fold(c[1])
            assert np.frombuffer(a, np.float32)[0] == np.float32(score) and np.frombuffer(b, np.int32)[0] == winner, (i, c)
            seen.add(("fold", winner >= 0))
        elif c[0] == 1:
            br, RH = tc.branch_of(c[1], c[2], c[3])
            assert np.frombuffer(a, np.int32)[0] == br and np.frombuffer(b, np.float32)[0] == RH, (i, c)
            seen.add(("branch", br))
        else:
            rule = tc.final_f if c[0] == 2 else tc.final_h
            want = rule([int(g) for g in c[1]], [float(x) for x in c[2]], c[3], 1.0, c[4])
            assert np.frombuffer(a, np.int32)[0] == want, (i, c, want)
            seen.add(("final", c[0], want >= 0))
    assert {("fold", True), ("fold", False), ("branch", 0), ("branch", 1), ("branch", 2), ("final", 2, True), ("final", 2, False),
            ("final", 3, True), ("final", 3, False)} <= seen
