// KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) on the device-resident BoW database of libmsorb
// (msorb_kf_database_*), written against the reference's own types by name (templates: this header compiles inside MS-SLAM,
// where KeyFrame / Frame / Map are the real classes, and in tests/dropin_kfdb_main.cc, where they are minimal stand-ins with
// the same member names).
//
//   ORB_SLAM3::msorb_host::KeyFrameDatabase<KeyFrame, Frame, Map>
//       add(pKF)                                  :39-45
//       erase(pKF)                                :47-66
//       clear()                                   :68-72
//       clearMap(pMap)                            :74-98
//       DetectRelocalizationCandidates(F, pMap)   :738-850
//       DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates)   :601-735 (MS-SLAM's variant: only sparsified,
//                                                 unconnected KeyFrames are listed)
//
// What runs where.  The inverted-file walk (:612-633, :746-761), the common-word counts and the L1 scores
// (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) are one device call; this class keeps entry id <-> shared_ptr<KeyFrame> (it
// holds the pointer, as the inverted file does), builds the `listed` mask from the members the reference tests, and writes
// mnRelocQuery / mnRelocWords / mRelocScore and mnPlaceRecognitionQuery / mnPlaceRecognitionWords / mPlaceRecognitionScore
// exactly as the reference leaves them, KeyFrames that share words without being listed included.  Everything from the
// covisibility loop on is the reference's statements over the reference's types.
//
// Differences to know about:
//   * erase removes exactly what add entered.  The reference walks the KeyFrame's CURRENT BowVector (:50), which in MS-SLAM is
//     the same thing: the database is filled in LoopClosing::DeleteOutdatedInfo (LoopClosing.cc:318-328) right after
//     KeyFrame::EraseBadDescriptor recomputed the vector, which is fixed from then on.
//   * There is one entry per KeyFrame: add of a KeyFrame that is already in is ignored (the reference would put it on every
//     list twice and count each of its words twice; MS-SLAM adds a KeyFrame once).
//   * The BowVector is read through GetBowVector() once, at add.
//   * mRelocScore is not initialised by the reference's constructors (KeyFrame.cc:34-35, :49) and DetectRelocalizationCandidates
//     reads it for neighbours it did not score in this query (:812-815): give it an initialiser where the class is defined.
//
// Use inside the reference: KeyFrameDatabase keeps its interface, holds one of these and forwards.
#ifndef MSORB_KEYFRAMEDATABASE_DEVICE_H
#define MSORB_KEYFRAMEDATABASE_DEVICE_H

#include <cstddef>
#include <cstdint>
#include <list>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "msorb.h"

namespace ORB_SLAM3 {
namespace msorb_host {
#ifndef MSORB_HOST_FAIL_CALL
#define MSORB_HOST_FAIL_CALL
// a failed call of the C ABI: the application's fatal-error callback first (msorb_set_fatal_callback), then std::runtime_error
[[noreturn]] inline void fail_call(const char* what) {
    const std::string msg = std::string(what) + ": " + msorb_last_error();
    msorb_notify_fatal(MSORB_E_HIP, msg.c_str());
    throw std::runtime_error(msg);
}
#endif

template <class KeyFrameT, class FrameT, class MapT>
class KeyFrameDatabase {
public:
    typedef std::shared_ptr<KeyFrameT> KeyFramePtr;

    // n_words = voc.size() (the reference sizes mvInvertedFile with it, :35)
    explicit KeyFrameDatabase(int n_words, int device = 0) {
        if (!msorb_abi_compatible(MSORB_ABI_VERSION)) {
            const std::string msg = "libmsorb.so has ABI " + std::to_string(msorb_abi_version()) + ", the host layer was compiled against " +
                                    std::to_string(MSORB_ABI_VERSION) + " (include/msorb.h)";
            msorb_notify_fatal(MSORB_E_INVALID, msg.c_str());
            throw std::runtime_error(msg);
        }
        if (msorb_kf_database_create(device, n_words, &db_) != MSORB_OK) fail_call("msorb_kf_database_create");
    }
    ~KeyFrameDatabase() { msorb_kf_database_destroy(db_); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    void add(KeyFramePtr pKF) {
        std::unique_lock<std::mutex> lock(mMutex);
        if (id_of_.count(pKF.get())) return;
        std::vector<int> word;
        std::vector<double> value;
        flatten(pKF->GetBowVector(), word, value);
        int id = -1;
        if (msorb_kf_database_add(db_, word.data(), value.data(), (int)word.size(), &id) != MSORB_OK) fail_call("msorb_kf_database_add");
        if (id >= (int)kf_of_.size()) kf_of_.resize((size_t)id + 1);
        kf_of_[id] = pKF;
        id_of_[pKF.get()] = id;
    }

    void erase(KeyFramePtr pKF) {
        std::unique_lock<std::mutex> lock(mMutex);
        auto it = id_of_.find(pKF.get());
        if (it == id_of_.end()) return;
        erase_id(it->second);
        id_of_.erase(it);
    }

    void clear() {
        std::unique_lock<std::mutex> lock(mMutex);
        if (msorb_kf_database_clear(db_) != MSORB_OK) fail_call("msorb_kf_database_clear");
        kf_of_.clear();
        id_of_.clear();
    }

    void clearMap(MapT* pMap) {
        std::unique_lock<std::mutex> lock(mMutex);
        for (int id = 0; id < (int)kf_of_.size(); id++) {
            KeyFramePtr pKFi = kf_of_[id];
            if (pKFi && pMap == pKFi->GetMap()) {
                id_of_.erase(pKFi.get());
                erase_id(id);
            }
        }
    }

    size_t size() const {
        std::unique_lock<std::mutex> lock(mMutex);
        return id_of_.size();
    }

    std::vector<KeyFramePtr> DetectRelocalizationCandidates(FrameT* F, MapT* pMap) {
        std::list<KeyFramePtr> lKFsSharingWords;
        std::vector<double> vScore;   // score(F->mBowVec, pKFi->GetBowVector()) of every listed KeyFrame, in list order
        int minCommonWords = 0;

        // Search all keyframes that share a word with current frame
        {
            std::unique_lock<std::mutex> lock(mMutex);
            Answer a;
            query(F->mBowVec, 0, [&](const KeyFramePtr& pKFi) { return pKFi->mnRelocQuery != F->mnId; }, a);
            for (int k = 0; k < a.n_listed; k++) {
                const KeyFramePtr& pKFi = kf_of_[a.entry[k]];
                pKFi->mnRelocWords = a.common[k];   // = 0, then ++ at every encounter (:755-759)
                pKFi->mnRelocQuery = F->mnId;
                lKFsSharingWords.push_back(pKFi);
                vScore.push_back(a.score[k]);
            }
            for (int k = a.n_listed; k < a.n_sharing; k++)   // already carries this query's id: only the ++ of :759
                kf_of_[a.entry[k]]->mnRelocWords += a.common[k];
            minCommonWords = a.min_common;                  // maxCommonWords*0.8f (:767-774)
        }
        if (lKFsSharingWords.empty()) return std::vector<KeyFramePtr>();

        std::list<std::pair<float, KeyFramePtr> > lScoreAndMatch;

        // Compute similarity score.
        size_t k = 0;
        for (typename std::list<KeyFramePtr>::iterator lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++, k++) {
            KeyFramePtr pKFi = *lit;

            if (pKFi->mnRelocWords > minCommonWords) {
                float si = (float)vScore[k];
                pKFi->mRelocScore = si;
                lScoreAndMatch.push_back(std::make_pair(si, pKFi));
            }
        }

        if (lScoreAndMatch.empty()) return std::vector<KeyFramePtr>();

        std::list<std::pair<float, KeyFramePtr> > lAccScoreAndMatch;
        float bestAccScore = 0;

        // Lets now accumulate score by covisibility
        for (typename std::list<std::pair<float, KeyFramePtr> >::iterator it = lScoreAndMatch.begin(), itend = lScoreAndMatch.end(); it != itend; it++) {
            KeyFramePtr pKFi = it->second;
            std::vector<KeyFramePtr> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);

            float bestScore = it->first;
            float accScore = bestScore;
            KeyFramePtr pBestKF = pKFi;
            for (typename std::vector<KeyFramePtr>::iterator vit = vpNeighs.begin(), vend = vpNeighs.end(); vit != vend; vit++) {
                KeyFramePtr pKF2 = *vit;
                if (pKF2->mnRelocQuery != F->mnId) continue;

                accScore += pKF2->mRelocScore;   // (of a neighbour below the threshold: what an earlier query left, :789 never resets)
                if (pKF2->mRelocScore > bestScore) {
                    pBestKF = pKF2;
                    bestScore = pKF2->mRelocScore;
                }
            }
            lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
            if (accScore > bestAccScore) bestAccScore = accScore;
        }

        // Return all those keyframes with a score higher than 0.75*bestScore
        float minScoreToRetain = 0.75f * bestAccScore;
        std::set<KeyFramePtr> spAlreadyAddedKF;
        std::vector<KeyFramePtr> vpRelocCandidates;
        vpRelocCandidates.reserve(lAccScoreAndMatch.size());
        for (typename std::list<std::pair<float, KeyFramePtr> >::iterator it = lAccScoreAndMatch.begin(), itend = lAccScoreAndMatch.end(); it != itend; it++) {
            const float& si = it->first;
            if (si > minScoreToRetain) {
                KeyFramePtr pKFi = it->second;
                if (pKFi->GetMap() != pMap) continue;
                if (!spAlreadyAddedKF.count(pKFi)) {
                    vpRelocCandidates.push_back(pKFi);
                    spAlreadyAddedKF.insert(pKFi);
                }
            }
        }

        return vpRelocCandidates;
    }

    void DetectNBestCandidates(KeyFramePtr pKF, std::vector<KeyFramePtr>& vpLoopCand, std::vector<KeyFramePtr>& vpMergeCand, int nNumCandidates) {
        std::list<KeyFramePtr> lKFsSharingWords;
        std::vector<double> vScore;
        std::set<KeyFramePtr> spConnectedKF;
        int minCommonWords = 0;
        // Search all keyframes that share a word with current frame
        {
            std::unique_lock<std::mutex> lock(mMutex);

            spConnectedKF = pKF->GetConnectedKeyFrames();

            Answer a;
            query(pKF->GetBowVector(), 1,
                  [&](const KeyFramePtr& pKFi) {
                      return pKFi->mnPlaceRecognitionQuery != pKF->mnId && pKFi->mbSparsified && !spConnectedKF.count(pKFi);
                  },
                  a);
            for (int k = 0; k < a.n_listed; k++) {
                const KeyFramePtr& pKFi = kf_of_[a.entry[k]];
                pKFi->mnPlaceRecognitionWords = a.common[k];
                pKFi->mnPlaceRecognitionQuery = pKF->mnId;
                lKFsSharingWords.push_back(pKFi);
                vScore.push_back(a.score[k]);
            }
            for (int k = a.n_listed; k < a.n_sharing; k++) {
                const KeyFramePtr& pKFi = kf_of_[a.entry[k]];
                if (pKFi->mnPlaceRecognitionQuery != pKF->mnId)
                    pKFi->mnPlaceRecognitionWords = 1;   // unsparsified or connected: reset to 0 at EVERY encounter, then ++ (:620-631)
                else
                    pKFi->mnPlaceRecognitionWords += a.common[k];
            }
            minCommonWords = a.min_common;   // maxCommonWords > 10 ? maxCommonWords*0.8f : maxCommonWords*0.6f (:639-650)
        }
        if (lKFsSharingWords.empty()) return;

        std::list<std::pair<float, KeyFramePtr> > lScoreAndMatch;

        // Compute similarity score.
        size_t k = 0;
        for (typename std::list<KeyFramePtr>::iterator lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++, k++) {
            KeyFramePtr pKFi = *lit;

            if (pKFi->mnPlaceRecognitionWords > minCommonWords) {
                float si = (float)vScore[k];
                pKFi->mPlaceRecognitionScore = si;
                lScoreAndMatch.push_back(std::make_pair(si, pKFi));
            } else
                pKFi->mPlaceRecognitionScore = 0;
        }

        if (lScoreAndMatch.empty()) return;

        std::list<std::pair<float, KeyFramePtr> > lAccScoreAndMatch;
        float bestAccScore = 0;

        // Lets now accumulate score by covisibility
        for (typename std::list<std::pair<float, KeyFramePtr> >::iterator it = lScoreAndMatch.begin(), itend = lScoreAndMatch.end(); it != itend; it++) {
            KeyFramePtr pKFi = it->second;
            std::vector<KeyFramePtr> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);

            float bestScore = it->first;
            float accScore = bestScore;
            KeyFramePtr pBestKF = pKFi;
            for (typename std::vector<KeyFramePtr>::iterator vit = vpNeighs.begin(), vend = vpNeighs.end(); vit != vend; vit++) {
                KeyFramePtr pKF2 = *vit;
                if (pKF2->mnPlaceRecognitionQuery != pKF->mnId) continue;

                accScore += pKF2->mPlaceRecognitionScore;
                if (pKF2->mPlaceRecognitionScore > bestScore) {
                    pBestKF = pKF2;
                    bestScore = pKF2->mPlaceRecognitionScore;
                }
            }
            lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
            if (accScore > bestAccScore) bestAccScore = accScore;
        }

        lAccScoreAndMatch.sort(compFirst);

        vpLoopCand.reserve(nNumCandidates);
        vpMergeCand.reserve(nNumCandidates);
        std::set<KeyFramePtr> spAlreadyAddedKF;
        size_t i = 0;
        typename std::list<std::pair<float, KeyFramePtr> >::iterator it = lAccScoreAndMatch.begin();
        while (i < lAccScoreAndMatch.size() && ((int)vpLoopCand.size() < nNumCandidates || (int)vpMergeCand.size() < nNumCandidates)) {
            KeyFramePtr pKFi = it->second;
            if (pKFi->isBad()) {
                i++;
                it++;
                continue;
            }

            if (!spAlreadyAddedKF.count(pKFi)) {
                if (pKF->GetMap() == pKFi->GetMap() && (int)vpLoopCand.size() < nNumCandidates) {
                    vpLoopCand.push_back(pKFi);
                } else if (!pKF->GetMap() && pKF->GetMap() != pKFi->GetMap() && (int)vpMergeCand.size() < nNumCandidates && !pKFi->GetMap()->IsBad()) {
                    vpMergeCand.push_back(pKFi);   // (the condition is the reference's, as written)
                }
                spAlreadyAddedKF.insert(pKFi);
            }
            i++;
            it++;
        }
    }

private:
    struct Answer {
        std::vector<int> entry, common;
        std::vector<double> score;
        int n_sharing = 0, n_listed = 0, max_common = 0, min_common = 0;
    };

    static bool compFirst(const std::pair<float, KeyFramePtr>& a, const std::pair<float, KeyFramePtr>& b) { return a.first > b.first; }

    template <class BowVectorT>
    static void flatten(const BowVectorT& v, std::vector<int>& word, std::vector<double>& value) {
        word.clear();
        value.clear();
        word.reserve(v.size());
        value.reserve(v.size());
        for (typename BowVectorT::const_iterator vit = v.begin(), vend = v.end(); vit != vend; vit++) {
            word.push_back((int)vit->first);
            value.push_back((double)vit->second);
        }
    }

    void erase_id(int id) {   // (mMutex is held)
        if (msorb_kf_database_erase(db_, id) != MSORB_OK) fail_call("msorb_kf_database_erase");
        kf_of_[id].reset();
    }

    // (mMutex is held: the ids and the members the mask is built from do not change under the call)
    template <class BowVectorT, class ListedT>
    void query(const BowVectorT& bow, int rule, ListedT listed, Answer& a) {
        std::vector<int> word;
        std::vector<double> value;
        flatten(bow, word, value);
        const int bound = (int)kf_of_.size();
        std::vector<uint8_t> mask((size_t)bound + 1, 0);
        for (int id = 0; id < bound; id++)
            if (kf_of_[id]) mask[id] = listed(kf_of_[id]) ? 1 : 0;
        a.entry.resize((size_t)bound + 1);
        a.common.resize((size_t)bound + 1);
        a.score.resize((size_t)bound + 1);
        if (msorb_kf_database_query(db_, word.data(), value.data(), (int)word.size(), mask.data(), rule, a.entry.data(), a.common.data(),
                                    a.score.data(), bound, &a.n_sharing, &a.n_listed, &a.max_common, &a.min_common, nullptr) != MSORB_OK)
            fail_call("msorb_kf_database_query");
    }

    mutable std::mutex mMutex;
    msorb_kf_database* db_ = nullptr;
    std::vector<KeyFramePtr> kf_of_;                  // by entry id; empty for an id that is free
    std::unordered_map<const KeyFrameT*, int> id_of_;
};

}  // namespace msorb_host
}  // namespace ORB_SLAM3

#endif
