// Plain C++ about two DBoW2::FeatureVectors and a match list, shared by every BoW-node search of bow_match.hip and free of HIP:
// the FeatureVector as CSR and its validation, the merge walk over the nodes two vectors share, the rotation-consistency
// filter, the candidate pick of the search whose geometric test lives with the caller, the split of a two-camera frame's
// vector by camera, the packing of the triangulation side.  (ORBmatcher.cc line numbers as in bow_match.hip.)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "matcher_rules.h"

namespace msorb {

struct FeatVec {  // DBoW2::FeatureVector as CSR
    int nodes;
    const int *node, *begin, *feat;
};

inline bool check_feature_vector(int n, const FeatVec& v, std::vector<uint8_t>& seen) {
    if (v.nodes < 0 || (v.nodes > 0 && (!v.node || !v.begin))) return false;
    if (v.nodes == 0) return true;
    if (v.begin[0] < 0) return false;
    for (int r = 0; r < v.nodes; r++) {
        if (v.begin[r + 1] < v.begin[r]) return false;
        if (r > 0 && v.node[r] <= v.node[r - 1]) return false;
    }
    if (v.begin[v.nodes] > v.begin[0] && !v.feat) return false;
    seen.assign((size_t)n, 0);
    for (int k = v.begin[0]; k < v.begin[v.nodes]; k++) {
        const int i = v.feat[k];
        if (i < 0 || i >= n || seen[i]) return false;
        seen[i] = 1;
    }
    return true;
}

// The merge walk of :239-243 / :385-392: visit(r1, r2, l1, l2) for the nodes both vectors hold with non-empty lists (rows r1 / r2,
// list lengths l1 / l2), ascending.  max_chunks grows to the 64-train chunks of the longest train list met (one bit per train in
// LDS); false when a train list has 1 << 20 entries or more (the kernels' key is dist << 20 | position), the walk ends there.
template <class Visit>
bool for_each_common_node(const FeatVec& a, const FeatVec& b, int& max_chunks, Visit visit) {
    int i = 0, j = 0;
    while (i < a.nodes && j < b.nodes) {
        if (a.node[i] == b.node[j]) {
            const int l1 = a.begin[i + 1] - a.begin[i], l2 = b.begin[j + 1] - b.begin[j];
            if (l1 > 0 && l2 > 0) {
                if (l2 >= (1 << 20)) return false;
                max_chunks = std::max(max_chunks, (l2 + 63) >> 6);
                visit(i, j, l1, l2);
            }
            i++; j++;
        } else if (a.node[i] < b.node[j]) i++;
        else j++;
    }
    return true;
}

// The rotation histogram and the ComputeThreeMaxima filter (:340-353 + :396-418, :1342-1354 + :1360-1381) over n entries:
// slot(k) = the place of entry k's match in `out`, -1 when entry k holds none; angles(k, a, b) = its two keypoint angles (asked
// only with check_orientation).  A match outside the three fullest bins, or whose bin is -1 (NaN / out-of-range angle: the
// reference asserts), is withdrawn: out[slot] = -1.  Returns the matches left.  The reference keeps 30 vectors in the order it
// visits the matches; only their 30 sizes enter ComputeThreeMaxima and every withdrawn match is withdrawn on its own, so the
// survivors do not depend on that order: a bin per entry and 30 counters do (with the vectors this cost 23 us per pair).
template <class Slot, class Angles>
int rotation_filter(int n, int check_orientation, int* out, Slot slot, Angles angles) {
    int kept = 0;
    if (!check_orientation) {
        for (int k = 0; k < n; k++) kept += slot(k) >= 0;
        return kept;
    }
    static thread_local std::vector<int8_t> bin_of;
    if ((int)bin_of.size() < n) bin_of.resize(n);
    int sizes[kHistoLength] = {0}, ind[3];
    for (int k = 0; k < n; k++) {
        bin_of[k] = -1;
        const int s = slot(k);
        if (s < 0) continue;
        float a, b;
        angles(k, a, b);
        const int bin = rotation_bin(a, b);
        if (bin >= 0) { bin_of[k] = (int8_t)bin; sizes[bin]++; }
        else out[s] = -1;
    }
    msorb_three_maxima(sizes, kHistoLength, ind);
    for (int k = 0; k < n; k++) {
        const int bin = bin_of[k];
        if (bin < 0) continue;
        if (bin == ind[0] || bin == ind[1] || bin == ind[2]) kept++;
        else out[slot(k)] = -1;
    }
    return kept;
}

// One (query, train) within the distance threshold, as node_candidates_kernel lists them (an int4): all candidates of a query one
// behind the other, the queries in the reference's visiting order.
struct NodeCand { int query, train, dist, pos; };

// SearchForTriangulation's scan (:1230-1358) over such a list: a query scans its node's trains in list order, keeps bestDist and
// takes a train when dist <= bestDist and the test passes — the passing unclaimed train of smallest distance, the LAST of equal
// ones.  Here: one query's candidates sorted by (distance, position descending), the first unclaimed one accept(query, train)
// passes is taken: match12[query] = train, claimed[train] = 1 (vbMatched2, :1212 / :1262 / :1345).  accept is a pure predicate.
template <class Accept>
void pick_candidates(const NodeCand* all, size_t n, uint8_t* claimed, int* match12, Accept accept) {
    std::vector<NodeCand> group;
    for (size_t k = 0, k_end; k < n; k = k_end) {
        for (k_end = k; k_end < n && all[k_end].query == all[k].query;) k_end++;
        group.assign(all + k, all + k_end);
        std::sort(group.begin(), group.end(),
                  [](const NodeCand& a, const NodeCand& b) { return a.dist != b.dist ? a.dist < b.dist : a.pos > b.pos; });
        for (const NodeCand& c : group) {
            if (claimed[c.train] || !accept(c.query, c.train)) continue;   // :1262, :1332
            match12[c.query] = c.train;
            claimed[c.train] = 1;
            break;
        }
    }
}

// A two-camera frame's FeatureVector split by camera (features < n_left are the left camera's): the node ids and the order
// inside a node stay, a node without features of a camera is not in that camera's vector.
struct OwnedFeatVec {
    std::vector<int> node, begin{0}, feat;
    FeatVec view() const { return FeatVec{(int)node.size(), node.data(), begin.data(), feat.data()}; }
};
struct CameraSplit { OwnedFeatVec left, right; };
inline CameraSplit split_by_camera(const FeatVec& v, int n_left) {
    CameraSplit s;
    for (int r = 0; r < v.nodes; r++) {
        const size_t l0 = s.left.feat.size(), r0 = s.right.feat.size();
        for (int k = v.begin[r]; k < v.begin[r + 1]; k++) (v.feat[k] < n_left ? s.left : s.right).feat.push_back(v.feat[k]);
        if (s.left.feat.size() > l0) { s.left.node.push_back(v.node[r]); s.left.begin.push_back((int)s.left.feat.size()); }
        if (s.right.feat.size() > r0) { s.right.node.push_back(v.node[r]); s.right.begin.push_back((int)s.right.feat.size()); }
    }
    return s;
}

// What triangulation_match_kernel reads per feature, each output optional (nullptr): xy[2n] = keypoint position (set 1),
// tr[4n] = (x, y, 100 * scale[octave], sigma2[octave]) (set 2, :1287 / :1332), flags[n] = on | stereo << 1.
inline void pack_triangulation_side(int n, const msorb_keypoint* kp, const float* scale, const float* sigma2, const uint8_t* on,
                                    const uint8_t* stereo, float* xy, float* tr, uint8_t* flags) {
    for (int i = 0; xy && i < n; i++) { xy[2 * i] = kp[i].x; xy[2 * i + 1] = kp[i].y; }
    for (int i = 0; tr && i < n; i++) {
        const int oct = kp[i].octave;
        tr[4 * i] = kp[i].x;
        tr[4 * i + 1] = kp[i].y;
        tr[4 * i + 2] = 100 * scale[oct];  // (int * float -> float)
        tr[4 * i + 3] = sigma2[oct];
    }
    for (int i = 0; flags && i < n; i++) flags[i] = (uint8_t)((on[i] ? 1 : 0) | (stereo[i] ? 2 : 0));
}

}  // namespace msorb
