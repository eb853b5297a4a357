// The yardstick of tools/kf_database_latency.cc, not code under test: KeyFrameDatabase's place-recognition query as the reference
// runs it on one host core, restated with the reference's containers — the inverted file a std::vector of std::list (one list per
// word, src/KeyFrameDatabase.cc:35-45), the BowVectors std::map<word, double>, the walk of :746-761 over the lists with a counter
// and a query id per entry, the threshold of :767-774, and for the entries above it the L1 score by the merge walk with
// lower_bound of Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68.  The covisibility part (:797-849) is the same host code on both
// sides of the comparison and is left out.
#pragma once
#include <cmath>
#include <list>
#include <map>
#include <vector>

namespace kfdb_host_ref {

typedef std::map<unsigned, double> BowVector;

struct Entry {
    BowVector bow;
    long query = -1;
    int words = 0;
    float score = 0;
};

inline double l1_score(const BowVector& v1, const BowVector& v2) {
    BowVector::const_iterator a = v1.begin(), b = v2.begin();
    double score = 0;
    while (a != v1.end() && b != v2.end()) {
        if (a->first == b->first) {
            const double vi = a->second, wi = b->second;
            score += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
            ++a;
            ++b;
        } else if (a->first < b->first)
            a = v1.lower_bound(b->first);
        else
            b = v2.lower_bound(a->first);
    }
    return -score / 2.0;
}

struct Database {
    std::vector<std::list<Entry*> > inverted;
    std::list<Entry> entries;
    explicit Database(int n_words) : inverted(n_words) {}
    void add(const int* word, const double* value, int n) {
        entries.emplace_back();
        Entry* e = &entries.back();
        for (int i = 0; i < n; i++) e->bow.insert(e->bow.end(), std::make_pair((unsigned)word[i], value[i]));
        for (int i = 0; i < n; i++) inverted[word[i]].push_back(e);
    }
    // -> how many entries were scored; *sharing = length of the list of entries sharing words
    int query(const BowVector& q, long query_id, int* sharing) {
        std::list<Entry*> sharing_words;
        for (BowVector::const_iterator vit = q.begin(); vit != q.end(); ++vit) {
            std::list<Entry*>& l = inverted[vit->first];
            for (std::list<Entry*>::iterator lit = l.begin(); lit != l.end(); ++lit) {
                Entry* e = *lit;
                if (e->query != query_id) {
                    e->words = 0;
                    e->query = query_id;
                    sharing_words.push_back(e);
                }
                e->words++;
            }
        }
        *sharing = (int)sharing_words.size();
        int max_common = 0;
        for (Entry* e : sharing_words)
            if (e->words > max_common) max_common = e->words;
        const int min_common = max_common * 0.8f;
        int scored = 0;
        for (Entry* e : sharing_words)
            if (e->words > min_common) {
                e->score = (float)l1_score(q, e->bow);
                scored++;
            }
        return scored;
    }
};

}  // namespace kfdb_host_ref
