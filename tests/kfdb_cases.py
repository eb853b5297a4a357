"""Synthetic place-recognition databases and a pure Python / numpy restatement of KeyFrameDatabase (shared by the CPU and the GPU
tests of the device-resident BoW database).

The restatement follows the reference statement by statement: src/KeyFrameDatabase.cc:39-98 (add / erase / clear / clearMap),
:601-735 (MS-SLAM's DetectNBestCandidates), :738-850 (DetectRelocalizationCandidates) and the L1 score of
Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68.  The inverted file is a list per word, the state the reference keeps on the
KeyFrames lives on KeyFrame objects, `float` is np.float32 and `double` a Python float (one add per common word).

One thing is chosen here: mRelocScore is not initialised by the reference's constructors (KeyFrame.cc:34-35, :49), so its first
read is indeterminate there; the stand-in starts it at 0."""
import bisect

import numpy as np

F32 = np.float32


class Map:
    def __init__(self, mnId, bad=False):
        self.mnId, self.bad = mnId, bad

    def IsBad(self):
        return self.bad


class KeyFrame:
    """The members KeyFrameDatabase reads and writes (KeyFrame.h), with the constructors' initial values (KeyFrame.cc:34-35, :49)."""

    def __init__(self, mnId, words, values, pMap=None, sparsified=True, bad=False):
        self.mnId = mnId
        self.words = [int(w) for w in words]        # DBoW2::BowVector = std::map<WordId, WordValue>: ascending word id
        self.values = [float(v) for v in values]
        self.mpMap, self.mbSparsified, self.mbBad = pMap, sparsified, bad
        self.neighbours = []                        # GetBestCovisibilityKeyFrames(10)
        self.connected = set()                      # GetConnectedKeyFrames()
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = 0, 0, F32(0)
        self.mnPlaceRecognitionQuery, self.mnPlaceRecognitionWords, self.mPlaceRecognitionScore = 0, 0, F32(0)

    def GetMap(self):
        return self.mpMap

    def isBad(self):
        return self.mbBad

    def members(self):
        return (self.mnRelocQuery, self.mnRelocWords, float(self.mRelocScore), self.mnPlaceRecognitionQuery,
                self.mnPlaceRecognitionWords, float(self.mPlaceRecognitionScore))


class Frame:
    def __init__(self, mnId, words, values):
        self.mnId, self.words, self.values = mnId, [int(w) for w in words], [float(v) for v in values]


def l1_score(w1, v1, w2, v2):
    """ScoringObject.cpp:23-68 -> the double it returns."""
    i, j, n1, n2 = 0, 0, len(w1), len(w2)
    score = 0.0
    while i < n1 and j < n2:
        vi, wi = v1[i], v2[j]
        if w1[i] == w2[j]:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif w1[i] < w2[j]:
            i = bisect.bisect_left(w1, w2[j], i)   # v1.lower_bound
        else:
            j = bisect.bisect_left(w2, w1[i], j)
    return -score / 2.0


class KeyFrameDatabase:
    def __init__(self, n_words, stale_reloc_score=True):
        self.n_words = n_words
        self.mvInvertedFile = {}                    # word -> list of KeyFrames (a std::list each; only the non-empty ones exist here)
        self.stale_reloc_score = stale_reloc_score  # False: what the result would be if unscored neighbours counted 0 (CPU tests only)

    # ---- :39-98
    def add(self, pKF):
        for w in pKF.words:
            self.mvInvertedFile.setdefault(w, []).append(pKF)

    def erase(self, pKF):
        for w in pKF.words:
            lKFs = self.mvInvertedFile.get(w, [])
            for k, x in enumerate(lKFs):
                if x is pKF:
                    del lKFs[k]
                    break

    def clear(self):
        self.mvInvertedFile = {}

    def clearMap(self, pMap):
        for w in self.mvInvertedFile:
            self.mvInvertedFile[w] = [x for x in self.mvInvertedFile[w] if x.GetMap() is not pMap]

    # ---- :738-850
    def DetectRelocalizationCandidates(self, F, pMap):
        lKFsSharingWords = []
        for w in F.words:
            for pKFi in self.mvInvertedFile.get(w, []):
                if pKFi.mnRelocQuery != F.mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = F.mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        if not lKFsSharingWords:
            return []
        maxCommonWords = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > maxCommonWords:
                maxCommonWords = pKFi.mnRelocWords
        minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        lScoreAndMatch = []
        scored = set()
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = F32(l1_score(F.words, F.values, pKFi.words, pKFi.values))
                pKFi.mRelocScore = si
                scored.add(pKFi)
                lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in pKFi.neighbours:
                if pKF2.mnRelocQuery != F.mnId:
                    continue
                s2 = pKF2.mRelocScore if (self.stale_reloc_score or pKF2 in scored) else F32(0)
                accScore = F32(accScore + s2)
                if s2 > bestScore:
                    pBestKF = pKF2
                    bestScore = s2
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        vpRelocCandidates = []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain:
                if pKFi.GetMap() is not pMap:
                    continue
                if pKFi not in spAlreadyAddedKF:
                    vpRelocCandidates.append(pKFi)
                    spAlreadyAddedKF.add(pKFi)
        return vpRelocCandidates

    # ---- :601-735
    def DetectNBestCandidates(self, pKF, nNumCandidates, info=None):
        """-> (vpLoopCand, vpMergeCand); info (a dict) receives maxCommonWords, minCommonWords, the scored list and the accumulated
        list for the tests that must see a tie or the 0.6f arm."""
        vpLoopCand, vpMergeCand = [], []
        lKFsSharingWords = []
        spConnectedKF = pKF.connected
        for w in pKF.words:
            for pKFi in self.mvInvertedFile.get(w, []):
                if pKFi.mnPlaceRecognitionQuery != pKF.mnId:
                    pKFi.mnPlaceRecognitionWords = 0
                    if pKFi.mbSparsified:
                        if pKFi not in spConnectedKF:
                            lKFsSharingWords.append(pKFi)
                            pKFi.mnPlaceRecognitionQuery = pKF.mnId
                pKFi.mnPlaceRecognitionWords += 1
        if not lKFsSharingWords:
            return vpLoopCand, vpMergeCand
        maxCommonWords = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnPlaceRecognitionWords > maxCommonWords:
                maxCommonWords = pKFi.mnPlaceRecognitionWords
        if maxCommonWords > 10:
            minCommonWords = int(F32(maxCommonWords) * F32(0.8))
        else:
            minCommonWords = int(F32(maxCommonWords) * F32(0.6))
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnPlaceRecognitionWords > minCommonWords:
                si = F32(l1_score(pKF.words, pKF.values, pKFi.words, pKFi.values))
                pKFi.mPlaceRecognitionScore = si
                lScoreAndMatch.append((si, pKFi))
            else:
                pKFi.mPlaceRecognitionScore = F32(0)
        if info is not None:
            info.update(maxCommonWords=maxCommonWords, minCommonWords=minCommonWords, scored=list(lScoreAndMatch), acc=[])
        if not lScoreAndMatch:
            return vpLoopCand, vpMergeCand
        lAccScoreAndMatch = []
        bestAccScore = F32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in pKFi.neighbours:
                if pKF2.mnPlaceRecognitionQuery != pKF.mnId:
                    continue
                accScore = F32(accScore + pKF2.mPlaceRecognitionScore)
                if pKF2.mPlaceRecognitionScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mPlaceRecognitionScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        lAccScoreAndMatch.sort(key=lambda p: -p[0])    # std::list::sort(compFirst): stable, descending
        if info is not None:
            info["acc"] = list(lAccScoreAndMatch)
        spAlreadyAddedKF = set()
        i = 0
        while i < len(lAccScoreAndMatch) and (len(vpLoopCand) < nNumCandidates or len(vpMergeCand) < nNumCandidates):
            pKFi = lAccScoreAndMatch[i][1]
            if pKFi.isBad():
                i += 1
                continue
            if pKFi not in spAlreadyAddedKF:
                if pKF.GetMap() is pKFi.GetMap() and len(vpLoopCand) < nNumCandidates:
                    vpLoopCand.append(pKFi)
                elif (not pKF.GetMap()) and pKF.GetMap() is not pKFi.GetMap() and len(vpMergeCand) < nNumCandidates and \
                        not pKFi.GetMap().IsBad():
                    vpMergeCand.append(pKFi)
                spAlreadyAddedKF.add(pKFi)
            i += 1
        return vpLoopCand, vpMergeCand


def expected_query(db, words, values, rule, listed=None, id_of=None):
    """What msorb_kf_database_query reports for this query on the restatement's inverted file, without touching any KeyFrame state.
    listed: predicate on a KeyFrame (None = all); id_of: KeyFrame -> entry id (default mnId).
    The walk of :612-633 / :746-761 meets an entry once per common word, in ascending word order, so the double is accumulated
    during the walk with exactly the additions of the merge walk of ScoringObject.cpp (tests hold the two together)."""
    id_of = id_of or (lambda kf: kf.mnId)
    order, count, acc = [], {}, {}
    for w, vi in zip(words, values):
        w, vi = int(w), float(vi)
        for kf in db.mvInvertedFile.get(w, []):
            if kf not in count:
                count[kf] = 0
                acc[kf] = 0.0
                order.append(kf)
            count[kf] += 1
            wi = kf.values[bisect.bisect_left(kf.words, w)]
            acc[kf] += abs(vi - wi) - abs(vi) - abs(wi)
    lst = [kf for kf in order if listed is None or listed(kf)]
    rest = sorted((kf for kf in order if not (listed is None or listed(kf))), key=id_of)
    mx = max([count[kf] for kf in lst], default=0)
    if rule == 0 or mx > 10:
        mn = int(F32(mx) * F32(0.8))
    else:
        mn = int(F32(mx) * F32(0.6))
    return dict(entry=np.array([id_of(kf) for kf in lst + rest], np.int32),
                common_words=np.array([count[kf] for kf in lst + rest], np.int32),
                score=np.array([-acc[kf] / 2.0 for kf in lst] + [0.0] * len(rest), np.float64),
                n_sharing=len(order), n_listed=len(lst), max_common_words=mx, min_common_words=mn)


# ------------------------------------------------------------------------------------------------------------------------------
# generator
# ------------------------------------------------------------------------------------------------------------------------------
class Trajectory:
    """A camera going `laps` times round a loop of landmarks: the KeyFrame at lap position p sees landmarks [p*step, p*step+span),
    one random word per landmark; a `noise` share of its observations is dropped and replaced by random words.  Values are
    count * idf, L1-normalised in double (what TemplatedVocabulary::transform leaves in a BowVector for TF_IDF / L1_NORM)."""

    def __init__(self, seed, n_kf, n_words=100000, span=300, step=12, laps=2, noise=0.15):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.n_kf, self.n_words, self.span, self.step, self.laps, self.noise = n_kf, n_words, span, step, laps, noise
        self.per_lap = (n_kf + laps - 1) // laps
        self.landmark_word = self.rng.integers(0, n_words, self.per_lap * step + span)
        self.idf = -np.log(self.rng.uniform(1e-4, 0.9, n_words))

    def bow(self, i):
        """BowVector of a view at trajectory index i (fresh noise at every call) -> (int32 words ascending, float64 values)."""
        p = (i % self.per_lap) * self.step
        w = self.landmark_word[p:p + self.span].copy()
        drop = self.rng.random(self.span) < self.noise
        w[drop] = self.rng.integers(0, self.n_words, int(drop.sum()))
        words, counts = np.unique(w, return_counts=True)
        v = counts * self.idf[words]
        return words.astype(np.int32), (v / v.sum()).astype(np.float64)

    def keyframes(self, pMap=None):
        kfs = []
        for i in range(self.n_kf):
            w, v = self.bow(i)
            kfs.append(KeyFrame(i, w, v, pMap))
        link_neighbours(kfs, list(range(self.n_kf)))
        return kfs


def link_neighbours(kfs, index):
    """kfs[index[t]] gets kfs[index[t +- 1..5]] as its GetBestCovisibilityKeyFrames(10), nearest first."""
    n = len(index)
    for t in range(n):
        nb = []
        for d in range(1, 6):
            for u in (t - d, t + d):
                if 0 <= u < n:
                    nb.append(kfs[index[u]])
        kfs[index[t]].neighbours = nb


def add_duplicates(kfs, n_dup, pMap=None):
    """KeyFrame N+j is an exact copy of KeyFrame j (equal counts, equal scores), its neighbours the copies of j's neighbours."""
    n = len(kfs)
    for j in range(n_dup):
        kfs.append(KeyFrame(n + j, kfs[j].words, kfs[j].values, pMap if pMap is not None else kfs[j].mpMap))
    for j in range(n_dup):
        kfs[n + j].neighbours = [kfs[n + x.mnId] for x in kfs[j].neighbours if x.mnId < n_dup]
    return kfs


def big_case(seed=0, n_kf=3000, n_queries=6, n_dup=40):
    """The 3000-KeyFrame two-lap database with exact duplicates added in permuted order, and held-out queries.
    -> (trajectory, kfs in ADD order, list of (words, values))"""
    tr = Trajectory(seed, n_kf)
    m = Map(0)
    kfs = add_duplicates(tr.keyframes(m), n_dup, m)
    order = tr.rng.permutation(len(kfs))
    queries = [tr.bow(int(i)) for i in tr.rng.integers(0, n_kf, n_queries)]
    return tr, [kfs[i] for i in order], queries


def reloc_sequence(seed, n_kf=600, laps=3, n_queries=40, stale=True):
    """600 KeyFrames on three laps and 40 consecutive held-out frames -> (database, kfs, frames, map)"""
    tr = Trajectory(seed, n_kf, n_words=100000, span=300, step=12, laps=laps)
    m = Map(0)
    kfs = tr.keyframes(m)
    db = KeyFrameDatabase(tr.n_words, stale_reloc_score=stale)
    for kf in kfs:
        db.add(kf)
    start = int(tr.rng.integers(0, tr.per_lap - n_queries))
    frames = [Frame(1000 + t, *tr.bow(start + t)) for t in range(n_queries)]
    return db, kfs, frames, m


def nbest_sequence(seed, n_kf=600, laps=3, n_dup=200, n_queries=40, n_unsparsified=60, n_bad=30):
    """The three-lap database plus exact duplicates in random add order, some KeyFrames unsparsified or bad, a second map, and the
    querying KeyFrames' neighbours on their own lap as their connected sets -> (database (its add_order: indices into kfs), kfs by mnId, querying KeyFrames)"""
    tr = Trajectory(seed, n_kf, n_words=100000, span=300, step=12, laps=laps)
    m0, m1 = Map(0), Map(1)
    kfs = add_duplicates(tr.keyframes(m0), n_dup, m0)
    rng = tr.rng
    for i in rng.choice(len(kfs), n_unsparsified, replace=False):
        kfs[i].mbSparsified = False
    for i in rng.choice(len(kfs), n_bad, replace=False):
        kfs[i].mbBad = True
    for i in rng.choice(len(kfs), 40, replace=False):
        kfs[i].mpMap = m1
    db = KeyFrameDatabase(tr.n_words)
    db.add_order = [int(i) for i in rng.permutation(len(kfs))]
    for i in db.add_order:
        db.add(kfs[i])
    start = int(rng.integers(0, tr.per_lap - n_queries))
    queries = []
    for t in range(n_queries):
        q = KeyFrame(5000 + t, *tr.bow(start + t), m0)
        here = tr.per_lap + start + t     # the querying KeyFrame travels on the second lap: its covisible KeyFrames are connected
        q.connected = {kfs[here + d] for d in range(-5, 6) if 0 <= here + d < n_kf}
        queries.append(q)
    return db, kfs, queries


def small_case(seed=3):
    """Twelve BowVectors of 8 words out of 40 (maxCommonWords <= 10: the 0.6f arm of :646-650), two of them equal (a score tie).
    -> (database, kfs, querying KeyFrame)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = Map(0)
    kfs = []
    for i in range(12):
        w = np.sort(rng.choice(40, 8, replace=False))
        v = rng.uniform(0.5, 2.0, 8)
        kfs.append(KeyFrame(i, w, v / v.sum(), m))
    kfs[7] = KeyFrame(7, kfs[2].words, kfs[2].values, m)
    link_neighbours(kfs, list(range(12)))
    db = KeyFrameDatabase(40)
    for kf in kfs:
        db.add(kf)
    own = kfs[2].words[:4]                       # four words of the twins, four that they do not have
    w = np.sort(np.concatenate([own, rng.choice(sorted(set(range(40)) - set(kfs[2].words)), 4, replace=False)]))
    v = rng.uniform(0.5, 2.0, 8)
    return db, kfs, KeyFrame(100, w, v / v.sum(), m)
