"""CPU-only tests of the device-resident BoW database's yardstick: the Python restatement of KeyFrameDatabase (tests/kfdb_cases.py)
against a second, definition-level formulation, the conditions the GPU tests rely on (asserted on the restatement alone), the host
header against stand-ins, and the declarations of the C ABI."""
import os
import re
import subprocess

import numpy as np
import pytest

import kfdb_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dense(n_words, words, values):
    d = np.zeros(n_words)
    d[np.asarray(words, np.int64)] = values
    return d


@pytest.fixture(scope="module")
def mid_case():
    tr = kc.Trajectory(5, 400, n_words=20000, span=300, step=12, laps=2)
    m = kc.Map(0)
    kfs = kc.add_duplicates(tr.keyframes(m), 30, m)
    order = [kfs[i] for i in tr.rng.permutation(len(kfs))]
    db = kc.KeyFrameDatabase(tr.n_words)
    for kf in order:
        db.add(kf)
    return tr, db, order, [tr.bow(i) for i in (7, 150, 333)]


def test_restatement_against_the_definitions(mid_case):
    """score = 1 - 1/2 |v - w|_1 on dense vectors (both L1-normalised) to 1e-12, counts = set intersections, list order = sort by
    (first common word, add order); and the walk-accumulated double equals the merge walk's bit for bit."""
    tr, db, order, queries = mid_case
    seq = {kf: k for k, kf in enumerate(order)}
    for qw, qv in queries:
        exp = kc.expected_query(db, qw, qv, 0)
        by_id = {kf.mnId: kf for kf in order}
        dq = _dense(tr.n_words, qw, qv)
        keys = []
        assert exp["n_listed"] == exp["n_sharing"] > 100
        for k in range(exp["n_sharing"]):
            kf = by_id[int(exp["entry"][k])]
            common = sorted(set(qw.tolist()) & set(kf.words))
            assert exp["common_words"][k] == len(common) > 0
            keys.append((common[0], seq[kf]))
            want = 1.0 - 0.5 * np.abs(dq - _dense(tr.n_words, kf.words, kf.values)).sum()
            assert abs(exp["score"][k] - want) < 1e-12
            merge = kc.l1_score(qw.tolist(), qv.tolist(), kf.words, kf.values)
            assert np.float64(merge).view(np.uint64) == exp["score"][k:k + 1].view(np.uint64)[0]
        assert keys == sorted(keys)
        sharing = {kf.mnId for kf in order if set(qw.tolist()) & set(kf.words)}
        assert sharing == set(exp["entry"].tolist())
        assert exp["max_common_words"] == exp["common_words"].max()
        assert exp["min_common_words"] == int(np.float32(exp["max_common_words"]) * np.float32(0.8))


def test_erase_and_readd_moves_a_keyframe_to_the_back(mid_case):
    tr, db, order, queries = mid_case
    qw, qv = queries[0]
    before = kc.expected_query(db, qw, qv, 0)["entry"].tolist()
    # a KeyFrame that precedes another one with the same first common word
    firsts = {}
    for kf in order:
        c = sorted(set(qw.tolist()) & set(kf.words))
        if c:
            firsts.setdefault(c[0], []).append(kf)
    group = next(g for g in firsts.values() if len(g) >= 2)
    mover = next(kf for kf in order if kf in group)
    db.erase(mover)
    assert mover.mnId not in kc.expected_query(db, qw, qv, 0)["entry"].tolist()
    db.add(mover)
    after = kc.expected_query(db, qw, qv, 0)["entry"].tolist()
    assert sorted(after) == sorted(before) and after != before
    others = [kf.mnId for kf in group if kf is not mover]
    assert all(after.index(mover.mnId) > after.index(o) for o in others)
    db.erase(mover)      # restore the add order for the other tests of the module
    for kf in order[order.index(mover) + 1:]:
        db.erase(kf)
    for kf in order[order.index(mover):]:
        db.add(kf)
    assert kc.expected_query(db, qw, qv, 0)["entry"].tolist() == before


def test_detect_relocalization_matches_the_definitions(mid_case):
    """One query on fresh state: the scored set is {common > min}, and the candidates follow from dense scores."""
    tr, db, order, queries = mid_case
    qw, qv = queries[1]
    exp = kc.expected_query(db, qw, qv, 0)
    F = kc.Frame(77, qw, qv)
    cand = db.DetectRelocalizationCandidates(F, order[0].GetMap())
    by_id = {kf.mnId: kf for kf in order}
    for k in range(exp["n_sharing"]):
        kf = by_id[int(exp["entry"][k])]
        assert kf.mnRelocQuery == 77 and kf.mnRelocWords == exp["common_words"][k]
        if exp["common_words"][k] > exp["min_common_words"]:
            assert kf.mRelocScore == np.float32(exp["score"][k])
        else:
            assert kf.mRelocScore == 0
    assert cand
    # the candidates lie near the query's place on one of the laps: > 80 % of the best count is within 5 steps of 4 % each, and the
    # best neighbour within 5 more
    assert all(abs(kf.mnId % tr.per_lap - 150 % tr.per_lap) <= 12 for kf in cand if kf.mnId < 400)
    for kf in order:     # leave no state behind
        kf.mnRelocQuery, kf.mnRelocWords, kf.mRelocScore = 0, 0, np.float32(0)


def test_stale_reloc_score_changes_a_result():
    """The covisibility loop of :809-821 adds the mRelocScore a PREVIOUS query left on neighbours below this query's threshold: on
    the 40-query sequence that changes the returned list on at least one query."""
    changed = 0
    for seed in (0, 1, 2):
        a = kc.reloc_sequence(seed, stale=True)
        b = kc.reloc_sequence(seed, stale=False)
        for Fa, Fb in zip(a[2], b[2]):
            ra = [kf.mnId for kf in a[0].DetectRelocalizationCandidates(Fa, a[3])]
            rb = [kf.mnId for kf in b[0].DetectRelocalizationCandidates(Fb, b[3])]
            changed += ra != rb
    assert changed >= 1, changed


def test_nbest_sequence_has_acc_score_ties_resolved_by_list_order():
    db, kfs, queries = kc.nbest_sequence(0)
    ties = 0
    found = 0
    for q in queries:
        info = {}
        loop, merge = db.DetectNBestCandidates(q, 3, info)
        found += len(loop)
        assert not merge      # the merge arm is `!pKF->GetMap() && ...`, as written: never taken with a map
        assert all(not kf.isBad() and kf.GetMap() is q.GetMap() and kf.mbSparsified and kf not in q.connected for kf in loop)
        acc = info.get("acc", [])
        for (s1, k1), (s2, k2) in zip(acc, acc[1:]):
            assert s1 >= s2
            ties += bool(s1 == s2 and k1 is not k2)
    assert ties >= 1 and found >= len(queries)
    # an unlisted sharing KeyFrame (unsparsified or connected) ends with its word counter at 1 and no query id
    q = queries[-1]
    touched = [kf for kf in kfs if (not kf.mbSparsified or kf in q.connected) and set(q.words) & set(kf.words)]
    assert touched and all(kf.mnPlaceRecognitionWords == 1 and kf.mnPlaceRecognitionQuery != q.mnId for kf in touched)


def test_small_case_takes_the_06_arm():
    db, kfs, q = kc.small_case()
    info = {}
    db.DetectNBestCandidates(q, 3, info)
    assert 0 < info["maxCommonWords"] <= 10
    assert info["minCommonWords"] == int(np.float32(info["maxCommonWords"]) * np.float32(0.6))
    assert info["minCommonWords"] != int(np.float32(info["maxCommonWords"]) * np.float32(0.8))
    exp = kc.expected_query(db, q.words, q.values, 1)
    assert (exp["max_common_words"], exp["min_common_words"]) == (info["maxCommonWords"], info["minCommonWords"])
    sc = [float(s) for s, _ in info["scored"]]
    assert len(sc) >= 2


def test_order_of_the_double_adds_is_visible(mid_case):
    """Summing the same terms back to front changes at least one double: a comparison of doubles sees a wrong order."""
    tr, db, order, queries = mid_case
    qw, qv = queries[2]
    exp = kc.expected_query(db, qw, qv, 0)
    by_id = {kf.mnId: kf for kf in order}
    q = dict(zip(qw.tolist(), qv.tolist()))
    differ = 0
    for k in np.argsort(-exp["common_words"])[:40]:
        kf = by_id[int(exp["entry"][k])]
        terms = [abs(q[w] - v) - abs(q[w]) - abs(v) for w, v in zip(kf.words, kf.values) if w in q]
        back = 0.0
        for t in reversed(terms):
            back += t
        differ += (-back / 2.0) != exp["score"][k]
    assert differ >= 1


def test_host_header_compiles_against_stand_ins():
    """ms-slam_amd/host/KeyFrameDatabase_device.h instantiated over the stand-in KeyFrame / Frame / Map of tests/dropin_kfdb_main.cc
    (syntax + template instantiation only: no GPU, no link)."""
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", f"-I{ROOT}/ms-slam_amd/host", f"-I{ROOT}/include",
                           os.path.join(ROOT, "tests", "dropin_kfdb_main.cc")])


def test_header_declares_the_database_entries(msorb_mod):
    hdr = open(os.path.join(ROOT, "include", "msorb.h")).read()
    names = ["msorb_kf_database_" + s for s in ("create", "destroy", "add", "erase", "clear", "info", "query")]
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in msorb_mod.EXPORTS and hasattr(msorb_mod.lib(), name)
    assert hasattr(msorb_mod, "KeyFrameDatabase")


def test_no_cpu_answer_without_a_device(msorb_mod):
    if msorb_mod.lib().msorb_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(msorb_mod.MsorbError) as e:
        msorb_mod.KeyFrameDatabase(1000)
    assert e.value.code == msorb_mod.E_NO_DEVICE
