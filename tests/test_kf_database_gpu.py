"""GPU parity: the device-resident BoW database (msorb_kf_database_*) through the C ABI against the Python restatement of
KeyFrameDatabase (tests/kfdb_cases.py): entries, list order, counts and thresholds equal, scores equal as bit patterns of the
doubles (a float comparison would not see a wrong order of the additions: tests/test_kf_database_cpu.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ms-slam_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))]
import bow_cases  # noqa: E402
import kfdb_cases as kc  # noqa: E402

pytestmark = pytest.mark.gpu


class Both:
    """The device database and the restatement fed with the same operations; entry id <-> KeyFrame as the host layer keeps it."""

    def __init__(self, n_words):
        import msorb
        self.dev = msorb.KeyFrameDatabase(n_words)
        self.ref = kc.KeyFrameDatabase(n_words)
        self.id = {}

    def add(self, kf):
        self.id[kf] = self.dev.add(np.array(kf.words, np.int32), np.array(kf.values, np.float64))
        self.ref.add(kf)
        return self.id[kf]

    def erase(self, kf):
        self.dev.erase(self.id.pop(kf))
        self.ref.erase(kf)

    def clear(self):
        self.dev.clear()
        self.ref.clear()
        self.id = {}

    def check(self, qw, qv, rule, listed=None):
        mask = None
        if listed is not None:
            mask = np.zeros(self.dev.info()["id_bound"], np.uint8)
            for kf, i in self.id.items():
                mask[i] = bool(listed(kf))
        got = self.dev.query(qw, qv, mask, rule)
        exp = kc.expected_query(self.ref, qw, qv, rule, listed, self.id.__getitem__)
        for k in ("n_sharing", "n_listed", "max_common_words", "min_common_words"):
            assert got[k] == exp[k], (k, got[k], exp[k])
        assert np.array_equal(got["entry"], exp["entry"])
        assert np.array_equal(got["common_words"], exp["common_words"])
        assert got["score"].dtype == np.float64 and got["score"].tobytes() == exp["score"].tobytes()   # bit patterns
        return got

    def close(self):
        self.dev.close()


def _listed_reloc(kf):        # some KeyFrames already carry this query's id (mnRelocQuery == F->mnId)
    return kf.mnId % 7 != 3


def _listed_nbest(kf):        # ... or are unsparsified / connected
    return kf.mnId % 7 != 3 and kf.mnId % 11 != 5 and not 100 <= kf.mnId < 111


@pytest.fixture(scope="module")
def big():
    tr, kfs, queries = kc.big_case()
    b = Both(tr.n_words)
    for kf in kfs:
        b.add(kf)
    yield b, kfs, queries
    b.close()


def test_every_query_of_the_3000_keyframe_case(big):
    b, kfs, queries = big
    assert b.dev.info()["n_entries"] == len(kfs) == 3040
    for qw, qv in queries:
        for rule, listed in ((0, None), (1, None), (0, _listed_reloc), (1, _listed_nbest)):
            got = b.check(qw, qv, rule, listed)
            assert got["n_sharing"] > 1000 and got["max_common_words"] > 150
            if listed is not None:
                assert 0 < got["n_listed"] < got["n_sharing"]
        scored = got["common_words"][:got["n_listed"]] > got["min_common_words"]
        assert 2 <= scored.sum() <= 60


def test_erase_readd_id_reuse_clear_and_flat_rows():
    tr = kc.Trajectory(5, 400, n_words=20000)
    m = kc.Map(0)
    kfs = kc.add_duplicates(tr.keyframes(m), 30, m)
    queries = [tr.bow(i) for i in (7, 150, 333)]
    b = Both(tr.n_words)
    try:
        for kf in kfs:
            b.add(kf)
        start = b.dev.info()
        assert start["n_entries"] == start["id_bound"] == 430 and start["rows_in_use"] == sum(len(kf.words) for kf in kfs)
        order0 = b.check(*queries[0], 0)["entry"].tolist()
        # erase + re-add: the KeyFrames move to the back of every list; the ids of the erased entries come back
        movers = [kfs[i] for i in (3, 8, 150, 151, 401, 10)]
        old_ids = {b.id[kf] for kf in movers}
        for kf in movers:
            b.erase(kf)
        assert b.dev.info()["n_entries"] == 424
        for q in queries:
            b.check(*q, 0)
            b.check(*q, 1, _listed_nbest)
        for kf in reversed(movers):
            b.add(kf)
        assert {b.id[kf] for kf in movers} == old_ids and b.dev.info()["id_bound"] == 430
        for q in queries:
            b.check(*q, 0)
            b.check(*q, 1, _listed_nbest)
        order1 = b.check(*queries[0], 0)["entry"].tolist()
        assert sorted(order0) == sorted(order1) and order0 != order1
        assert b.dev.info()["rows_in_use"] == start["rows_in_use"]
        # add / erase cycles with rows of changing length: the arena's use comes back to where it was
        for cycle in range(30):
            extra = [kc.KeyFrame(1000 + cycle * 10 + j, *tr.bow(int(tr.rng.integers(0, 400)))) for j in range(8)]
            gone = [kfs[int(i)] for i in tr.rng.choice(len(kfs), 5, replace=False)]
            for kf in gone:
                b.erase(kf)
            for kf in extra:
                b.add(kf)
            if cycle % 10 == 0:
                b.check(*queries[1], 0)
            for kf in extra:
                b.erase(kf)
            for kf in gone:
                b.add(kf)
        end = b.dev.info()
        assert end["rows_in_use"] == start["rows_in_use"] and end["n_entries"] == 430 and end["id_bound"] <= 438
        assert end["rows_reserved"] <= 2 * start["rows_reserved"] + 8192
        b.check(*queries[2], 1)
        # clear: nothing is met any more, ids start again
        b.clear()
        assert b.dev.info()["n_entries"] == b.dev.info()["id_bound"] == b.dev.info()["rows_in_use"] == 0
        assert b.check(*queries[0], 0)["n_sharing"] == 0
        assert b.add(kfs[5]) == 0 and b.add(kfs[6]) == 1
        for kf in kfs[20:200]:
            b.add(kf)
        for q in queries:
            b.check(*q, 0, _listed_reloc)
    finally:
        b.close()


def test_empty_query_empty_database_and_nothing_shared():
    rng = np.random.Generator(np.random.PCG64(4))
    b = Both(1000)
    try:
        w = np.arange(0, 300, 3, dtype=np.int32)
        v = np.full(len(w), 1.0 / len(w))
        got = b.check(w, v, 0)                                           # empty database
        assert got["n_sharing"] == got["n_listed"] == got["max_common_words"] == got["min_common_words"] == 0
        for i in range(20):
            ww = np.sort(rng.choice(np.arange(0, 300), 40, replace=False))
            vv = rng.random(40)
            b.add(kc.KeyFrame(i, ww, vv / vv.sum()))
        b.add(kc.KeyFrame(20, [], []))                                   # an entry without words is never met
        assert b.check(w, v, 1)["n_sharing"] > 0
        assert b.check(np.zeros(0, np.int32), np.zeros(0), 0)["n_sharing"] == 0          # empty query
        far = np.arange(500, 700, 2, dtype=np.int32)
        assert b.check(far, np.full(len(far), 0.01), 1)["n_sharing"] == 0                 # a query sharing nothing
    finally:
        b.close()


def test_small_case_thresholds_and_ties():
    ref, kfs, q = kc.small_case()
    b = Both(40)
    try:
        for kf in kfs:
            b.add(kf)
        got = b.check(np.array(q.words, np.int32), np.array(q.values), 1)
        assert 0 < got["max_common_words"] <= 10
        assert got["min_common_words"] == int(np.float32(got["max_common_words"]) * np.float32(0.6))
        s = {int(e): x for e, x in zip(got["entry"], got["score"])}
        assert s[b.id[kfs[2]]] == s[b.id[kfs[7]]]
        b.check(np.array(q.words, np.int32), np.array(q.values), 0)
    finally:
        b.close()


def test_entry_and_query_longer_than_the_lds_table():
    """20 000 words each: the query's table does not fit a workgroup's LDS (12 B per word) and is searched in global memory; the
    entry spans hundreds of 64-word steps of one wavefront.  The queries of 9 000 and 13 000 words take more than 64 KB of LDS."""
    rng = np.random.Generator(np.random.PCG64(9))
    n_words = 200000
    b = Both(n_words)

    def vec(n, pool=None):
        w = np.sort(rng.choice(n_words if pool is None else pool, n, replace=False)).astype(np.int32)
        v = rng.random(n) + 0.01
        return w, v / v.sum()
    try:
        long_kf = kc.KeyFrame(0, *vec(20000))
        b.add(long_kf)
        for i in range(1, 60):
            b.add(kc.KeyFrame(i, *vec(int(rng.integers(50, 3000)))))
        b.add(kc.KeyFrame(60, *vec(10000, np.array(long_kf.words))))    # a subset of the long entry's words
        for n in (20000, 13000, 9000, 5000, 300):
            qw, qv = vec(n)
            got = b.check(qw, qv, 0)
            assert got["n_sharing"] >= 30
            b.check(qw, qv, 1, lambda kf: kf.mnId % 3 != 1)
        qw, qv = vec(20000, np.array(sorted(set(long_kf.words[::2]) | set(rng.choice(n_words, 12000).tolist()))))
        got = b.check(qw, qv, 0)
        assert got["max_common_words"] > 5000
    finally:
        b.close()


def test_bow_vectors_of_the_device_transform():
    """BowVectors from msorb.Vocabulary.transform go in, the restatement is fed by OracleVocabulary.transform."""
    import msorb
    import orb_oracle
    voc = bow_cases.make_vocabulary(11, k=10, L=3)
    args = (voc["k"], voc["L"], 0, 0, voc["parent"], voc["is_leaf"], voc["descriptors"], voc["weights"])
    dev_voc, orc = msorb.Vocabulary(*args), orb_oracle.OracleVocabulary(*args)
    db = msorb.KeyFrameDatabase(dev_voc.n_words)
    ref = kc.KeyFrameDatabase(dev_voc.n_words)
    try:
        base = bow_cases.make_features(100, voc, 1200)
        rng = np.random.Generator(np.random.PCG64(2))
        ids = {}
        for i in range(40):
            feats = base.copy()
            swap = rng.random(len(feats)) < 0.1 + 0.02 * i
            feats[swap] = bow_cases.make_features(200 + i, voc, int(swap.sum()))
            d, o = dev_voc.transform(feats), orc.transform(feats)
            kf = kc.KeyFrame(i, o["bow_word"], o["bow_value"])
            ids[kf] = db.add(d["bow_word"], d["bow_value"])
            ref.add(kf)
        d, o = dev_voc.transform(base), orc.transform(base)
        for rule in (0, 1):
            got = db.query(d["bow_word"], d["bow_value"], None, rule)
            exp = kc.expected_query(ref, o["bow_word"], o["bow_value"], rule, None, ids.__getitem__)
            assert got["n_sharing"] == exp["n_sharing"] == 40 and got["max_common_words"] == exp["max_common_words"] > 100
            assert got["min_common_words"] == exp["min_common_words"]
            assert np.array_equal(got["entry"], exp["entry"]) and np.array_equal(got["common_words"], exp["common_words"])
            assert got["score"].tobytes() == exp["score"].tobytes()
    finally:
        db.close()
        dev_voc.close()


def test_refused_inputs_leave_the_database_intact(big):
    import msorb
    b, kfs, queries = big
    qw, qv = queries[0]
    before = b.dev.info()
    good = b.check(qw, qv, 0)
    bad_sets = [(qw[::-1].copy(), qv), (np.concatenate([qw[:5], qw[4:]]), np.concatenate([qv[:5], qv[4:]])),
                (np.concatenate([qw, [b.dev.n_words]]).astype(np.int32), np.concatenate([qv, [0.1]])),
                (np.concatenate([[-1], qw]).astype(np.int32), np.concatenate([[0.1], qv]))]
    for w, v in bad_sets:
        with pytest.raises(msorb.MsorbError) as e:
            b.dev.add(w, v)
        assert e.value.code == msorb.E_INVALID
        with pytest.raises(msorb.MsorbError) as e:
            b.dev.query(w, v)
        assert e.value.code == msorb.E_INVALID
    with pytest.raises(msorb.MsorbError) as e:
        b.dev.query(qw, qv, rule=2)
    assert e.value.code == msorb.E_INVALID
    for cap in (0, 1, good["n_sharing"] - 1):
        with pytest.raises(msorb.MsorbError) as e:
            b.dev.query(qw, qv, capacity=cap)
        assert e.value.code == msorb.E_CAPACITY and e.value.n_sharing == good["n_sharing"]
    assert b.dev.query(qw, qv, capacity=good["n_sharing"])["n_sharing"] == good["n_sharing"]
    for bad_id in (-1, before["id_bound"], 10 ** 6):
        with pytest.raises(msorb.MsorbError) as e:
            b.dev.erase(bad_id)
        assert e.value.code == msorb.E_INVALID
    assert b.dev.info() == before
    again = b.check(qw, qv, 0)
    assert again["score"].tobytes() == good["score"].tobytes() and np.array_equal(again["entry"], good["entry"])
    kf = kfs[17]                                    # an erased id is unknown until an add hands it out again
    dead = b.id[kf]
    b.erase(kf)
    with pytest.raises(msorb.MsorbError) as e:
        b.dev.erase(dead)
    assert e.value.code == msorb.E_INVALID
    assert b.add(kf) == dead
    b.check(qw, qv, 1)
