// Wall time of one place-recognition query on the device-resident BoW database, three ways in ONE process, in alternating blocks
// (order reversed every round), median of block medians with the spread:
//   abi            msorb_kf_database_query through the C ABI (upload of the query, one kernel, read-back, host ordering)
//   host_template  msorb_host::KeyFrameDatabase::DetectRelocalizationCandidates (mask, the query, the members, the covisibility part)
//   host_core      the same query by the inverted-file restatement of the reference on one host core (kf_database_host_ref.h),
//                  up to the scores
// on a synthetic multi-lap map (entries of ~`span` words; tests/kfdb_cases.py describes the model).  Prints one JSON line.
//   kf_database_latency <n_entries> <query_span> [rounds=8] [block=40]
// Built and driven by tools/kf_database_latency.py.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "KeyFrameDatabase_device.h"
#include "kf_database_host_ref.h"

namespace ORB_SLAM3 {
struct Map {
    bool IsBad() { return false; }
};
struct Frame {
    long unsigned int mnId = 0;
    kfdb_host_ref::BowVector mBowVec;
};
struct KeyFrame {
    long unsigned int mnId = 0, mnRelocQuery = 0, mnPlaceRecognitionQuery = 0;
    int mnRelocWords = 0, mnPlaceRecognitionWords = 0;
    float mRelocScore = 0, mPlaceRecognitionScore = 0;
    bool mbSparsified = true;
    kfdb_host_ref::BowVector mBowVec;
    Map* mpMap = nullptr;
    std::vector<std::shared_ptr<KeyFrame> > neighbours;
    const kfdb_host_ref::BowVector& GetBowVector() { return mBowVec; }
    Map* GetMap() { return mpMap; }
    bool isBad() { return false; }
    std::vector<std::shared_ptr<KeyFrame> > GetBestCovisibilityKeyFrames(const int&) { return neighbours; }
    std::set<std::shared_ptr<KeyFrame> > GetConnectedKeyFrames() { return std::set<std::shared_ptr<KeyFrame> >(); }
};
}  // namespace ORB_SLAM3

typedef std::shared_ptr<ORB_SLAM3::KeyFrame> KFPtr;

namespace {
const int kWords = 100000, kStep = 12;
const double kNoise = 0.15;

struct World {
    std::mt19937_64 rng;
    std::vector<int> landmark_word;
    std::vector<double> idf;
    int per_lap;
    World(int n_entries, int laps, int max_span) : rng(12345), per_lap((n_entries + laps - 1) / laps) {
        landmark_word.resize((size_t)per_lap * kStep + max_span);
        for (int& w : landmark_word) w = (int)(rng() % kWords);
        idf.resize(kWords);
        std::uniform_real_distribution<double> u(1e-4, 0.9);
        for (double& x : idf) x = -std::log(u(rng));
    }
    void bow(int i, int span, std::vector<int>& word, std::vector<double>& value) {
        std::map<int, int> count;
        std::uniform_real_distribution<double> u(0, 1);
        const size_t p = (size_t)(i % per_lap) * kStep;
        for (int k = 0; k < span; k++) count[u(rng) < kNoise ? (int)(rng() % kWords) : landmark_word[p + k]]++;
        word.clear();
        value.clear();
        double sum = 0;
        for (const auto& kv : count) { word.push_back(kv.first); value.push_back(kv.second * idf[kv.first]); sum += value.back(); }
        for (double& v : value) v /= sum;
    }
};

double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v.empty() ? 0 : v[v.size() / 2];
}
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const int n_entries = std::atoi(argv[1]), q_span = std::atoi(argv[2]);
    const int rounds = argc > 3 ? std::atoi(argv[3]) : 8, block = argc > 4 ? std::atoi(argv[4]) : 40;
    const int span = 300, n_queries = 16;
    World world(n_entries, 2, std::max(span, q_span));
    ORB_SLAM3::Map map;
    try {
        msorb_kf_database* db = nullptr;
        if (msorb_kf_database_create(0, kWords, &db) != MSORB_OK) throw std::runtime_error(msorb_last_error());
        ORB_SLAM3::msorb_host::KeyFrameDatabase<ORB_SLAM3::KeyFrame, ORB_SLAM3::Frame, ORB_SLAM3::Map> tdb(kWords);
        kfdb_host_ref::Database ref(kWords);
        std::vector<KFPtr> kfs(n_entries);
        std::vector<int> w;
        std::vector<double> v;
        size_t total_words = 0;
        for (int i = 0; i < n_entries; i++) {
            world.bow(i, span, w, v);
            total_words += w.size();
            int id = -1;
            if (msorb_kf_database_add(db, w.data(), v.data(), (int)w.size(), &id) != MSORB_OK) throw std::runtime_error(msorb_last_error());
            ref.add(w.data(), v.data(), (int)w.size());
            kfs[i] = std::make_shared<ORB_SLAM3::KeyFrame>();
            kfs[i]->mnId = (long unsigned int)i;
            kfs[i]->mpMap = &map;
            for (size_t k = 0; k < w.size(); k++) kfs[i]->mBowVec.insert(kfs[i]->mBowVec.end(), std::make_pair((unsigned)w[k], v[k]));
        }
        for (int i = 0; i < n_entries; i++) {
            for (int d = 1; d <= 5; d++)
                for (int u : {i - d, i + d})
                    if (u >= 0 && u < n_entries) kfs[i]->neighbours.push_back(kfs[u]);
            tdb.add(kfs[i]);
        }
        std::vector<std::vector<int> > qw(n_queries);
        std::vector<std::vector<double> > qv(n_queries);
        std::vector<kfdb_host_ref::BowVector> qb(n_queries);
        size_t query_words = 0;
        for (int q = 0; q < n_queries; q++) {
            world.bow((int)(world.rng() % n_entries), q_span, qw[q], qv[q]);
            query_words += qw[q].size();
            for (size_t k = 0; k < qw[q].size(); k++) qb[q].insert(qb[q].end(), std::make_pair((unsigned)qw[q][k], qv[q][k]));
        }
        std::vector<int> entry(n_entries), common(n_entries);
        std::vector<double> score(n_entries);
        int ns = 0, nl = 0, mx = 0, mn = 0;
        long next_id = 1;
        std::vector<double> kernel_ms;
        double sharing_sum = 0, scored_sum = 0, candidates_sum = 0;
        int disagree = 0;
        auto run_abi = [&](int q) {
            float ms = 0;
            if (msorb_kf_database_query(db, qw[q].data(), qv[q].data(), (int)qw[q].size(), nullptr, 0, entry.data(), common.data(), score.data(),
                                        n_entries, &ns, &nl, &mx, &mn, &ms) != MSORB_OK)
                throw std::runtime_error(msorb_last_error());
            kernel_ms.push_back(ms);
        };
        auto run_template = [&](int q) {
            ORB_SLAM3::Frame F;
            F.mnId = (long unsigned int)next_id++;
            F.mBowVec = qb[q];
            candidates_sum += (double)tdb.DetectRelocalizationCandidates(&F, &map).size();
        };
        int ref_sharing = 0, ref_scored = 0;
        auto run_ref = [&](int q) { ref_scored = ref.query(qb[q], next_id++, &ref_sharing); };
        // warm-up of every shape + agreement of the device and the host-core yardstick on what they count
        for (int q = 0; q < n_queries; q++) {
            run_abi(q);
            run_template(q);
            run_ref(q);
            int scored = 0;
            for (int k = 0; k < nl; k++) scored += common[k] > mn;
            disagree += ns != ref_sharing || scored != ref_scored;
            sharing_sum += ns;
            scored_sum += scored;
        }
        kernel_ms.clear();
        candidates_sum = 0;
        const char* names[3] = {"abi", "host_template", "host_core"};
        std::vector<double> block_medians[3];
        int calls = 0;
        for (int r = 0; r < rounds; r++)
            for (int s = 0; s < 3; s++) {
                const int m = r % 2 ? 2 - s : s;
                std::vector<double> t;
                for (int c = 0; c < block; c++) {
                    const int q = (calls++) % n_queries;
                    const double t0 = now_ms();
                    if (m == 0) run_abi(q);
                    else if (m == 1) run_template(q);
                    else run_ref(q);
                    t.push_back(now_ms() - t0);
                }
                block_medians[m].push_back(median(t));
            }
        std::printf("{\"n_entries\": %d, \"words_per_entry\": %.1f, \"query_span\": %d, \"words_per_query\": %.1f, \"rounds\": %d, \"block_calls\": %d, "
                    "\"sharing_per_query\": %.1f, \"scored_per_query\": %.1f, \"candidates_per_query\": %.2f, \"device_and_host_core_disagree\": %d, "
                    "\"abi_kernel_ms_median\": %.4f",
                    n_entries, (double)total_words / n_entries, q_span, (double)query_words / n_queries, rounds, block, sharing_sum / n_queries,
                    scored_sum / n_queries, candidates_sum / std::max(1, rounds * block), disagree, median(kernel_ms));
        for (int m = 0; m < 3; m++) {
            const std::vector<double>& b = block_medians[m];
            std::printf(", \"%s\": {\"median_ms\": %.4f, \"spread_ms\": %.4f, \"block_medians_ms\": [", names[m], median(b),
                        *std::max_element(b.begin(), b.end()) - *std::min_element(b.begin(), b.end()));
            for (size_t k = 0; k < b.size(); k++) std::printf("%s%.4f", k ? ", " : "", b[k]);
            std::printf("]}");
        }
        std::printf("}\n");
        msorb_kf_database_destroy(db);
        for (KFPtr& p : kfs) p->neighbours.clear();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "kf_database_latency: %s\n", e.what());
        return 3;
    }
    return 0;
}
