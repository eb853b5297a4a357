// ms-slam_amd/csrc/bow_pairs.h on the CPU, against restatements of the reference's loops written here, statement by statement,
// none of them taken from the header under test:
//   merge walk        a naive set intersection of the two vectors' node ids;
//   rotation filter   rotHist[30] of vectors filled in a visiting order (ORBmatcher.cc:340-353 / :1343-1353), ComputeThreeMaxima
//                     (:2277-2318), the entries of every other bin withdrawn (:396-418 / :1370-1387) — on a DRAWN visiting order,
//                     since the filter claims that the order does not matter; an entry the reference would assert on (its bin
//                     outside [0, 30)) is withdrawn;
//   candidate pick    the running-minimum scan with `dist > bestDist -> continue` (:1252-1341) under a drawn predicate;
//   camera split      a per-camera filter of every node's list;
//   packing           the two loops the function replaced.
// The program counts how often the cases that make each rule bite occur and fails when one of them is below 10 % of the scenes.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>
#include <vector>

#include "bow_pairs.h"

using namespace msorb;

#define CHECK(c)                                                                                     \
    do {                                                                                             \
        if (!(c)) { std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, g_where); std::exit(1); } \
    } while (0)
static char g_where[128] = "";

// The library's ComputeThreeMaxima lives in matcher_host.hip (msorb_three_maxima, checked by test_matcher_cpu.py) and is not
// linked here: this stand-in serves the header; the restatement below has its own, written over the 30 vectors.
extern "C" int msorb_three_maxima(const int* s, int L, int* ind) {
    int m[3] = {0, 0, 0};
    ind[0] = ind[1] = ind[2] = -1;
    for (int i = 0; i < L; i++) {
        int at = s[i] > m[0] ? 0 : s[i] > m[1] ? 1 : s[i] > m[2] ? 2 : 3;
        for (int k = 2; k > at; k--) { m[k] = m[k - 1]; ind[k] = ind[k - 1]; }
        if (at < 3) { m[at] = s[i]; ind[at] = i; }
    }
    if (m[1] < 0.1f * (float)m[0]) ind[1] = ind[2] = -1;
    else if (m[2] < 0.1f * (float)m[0]) ind[2] = -1;
    return 0;
}

struct Rng {   // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    float unit() { return (float)(next() >> 40) / (float)(1 << 24); }
    bool chance(float p) { return unit() < p; }
};

struct Share {
    const char* name;
    int hits = 0, scenes = 0;
    void print_and_check() const {
        std::printf("  %-58s %5.1f %% of %d\n", name, scenes ? 100.0 * hits / scenes : 0.0, scenes);
        if (!(scenes > 0 && hits * 10 >= scenes)) { std::printf("FAILED: share below 10 %%: %s\n", name); std::exit(1); }
    }
};

// ---------------------------------------------------------------------------------------------------------------- merge walk
struct Vec {
    std::vector<int> node, begin, feat;
    FeatVec view() const { return FeatVec{(int)node.size(), node.data(), begin.data(), feat.data()}; }
};
// node ids from `ids` kept with probability p, list lengths from `len()`, the lists behind begin0 unused entries
template <class Len>
static Vec draw_vec(Rng& g, const std::vector<int>& ids, float p, int begin0, Len len) {
    Vec v;
    v.begin.push_back(begin0);
    v.feat.assign(begin0, -7);
    for (int id : ids) {
        if (!g.chance(p)) continue;
        v.node.push_back(id);
        for (int k = len(); k > 0; k--) v.feat.push_back((int)v.feat.size() - begin0);
        v.begin.push_back((int)v.feat.size());
    }
    return v;
}
struct Visit { int r1, r2, l1, l2; };
static void test_merge_walk() {
    Share s_empty_list{"merge walk: a shared node with an empty list"}, s_begin0{"merge walk: begin[0] > 0"},
        s_one_empty{"merge walk: one vector empty"}, s_disjoint{"merge walk: no common node"}, s_chunks{"merge walk: a train list over 64"};
    Rng g{11};
    const int scenes = 2000;
    for (int sc = 0; sc < scenes; sc++) {
        std::snprintf(g_where, sizeof g_where, "merge walk scene %d", sc);
        std::vector<int> ids;
        for (int id = g.below(4); id < 120; id += 1 + g.below(4)) ids.push_back(id);
        const int kind = sc % 5;   // 1: one vector empty, 2: disjoint
        auto len = [&] { return g.chance(0.2f) ? 0 : g.chance(0.08f) ? 60 + g.below(80) : 1 + g.below(6); };
        Vec a = draw_vec(g, ids, kind == 1 && (sc & 8) ? 0.0f : 0.6f, g.chance(0.4f) ? 1 + g.below(5) : 0, len);
        Vec b = draw_vec(g, ids, kind == 1 && !(sc & 8) ? 0.0f : 0.6f, g.chance(0.4f) ? 1 + g.below(5) : 0, len);
        if (kind == 2) for (int& id : b.node) id += 1000;
        // naive: the ids both hold, ascending; the rows by search
        std::set<int> sa(a.node.begin(), a.node.end()), sb(b.node.begin(), b.node.end());
        std::vector<Visit> want;
        int want_chunks = 1;
        bool empty_list = false, common = false;
        for (int id : sa) {
            if (!sb.count(id)) continue;
            common = true;
            const int r1 = (int)(std::find(a.node.begin(), a.node.end(), id) - a.node.begin());
            const int r2 = (int)(std::find(b.node.begin(), b.node.end(), id) - b.node.begin());
            const int l1 = a.begin[r1 + 1] - a.begin[r1], l2 = b.begin[r2 + 1] - b.begin[r2];
            if (l1 == 0 || l2 == 0) { empty_list = true; continue; }
            want.push_back({r1, r2, l1, l2});
            want_chunks = std::max(want_chunks, (l2 + 63) / 64);
        }
        std::vector<Visit> got;
        int chunks = 1;
        CHECK(for_each_common_node(a.view(), b.view(), chunks, [&](int r1, int r2, int l1, int l2) { got.push_back({r1, r2, l1, l2}); }));
        CHECK(got.size() == want.size() && chunks == want_chunks);
        for (size_t i = 0; i < got.size(); i++)
            CHECK(got[i].r1 == want[i].r1 && got[i].r2 == want[i].r2 && got[i].l1 == want[i].l1 && got[i].l2 == want[i].l2);
        s_empty_list.hits += empty_list; s_begin0.hits += a.begin[0] > 0 || b.begin[0] > 0;
        s_one_empty.hits += a.node.empty() != b.node.empty(); s_disjoint.hits += !common && !a.node.empty() && !b.node.empty();
        s_chunks.hits += want_chunks > 1;
        for (Share* s : {&s_empty_list, &s_begin0, &s_one_empty, &s_disjoint, &s_chunks}) s->scenes++;
    }
    // a train list of 1 << 20 entries is refused (the kernels' key is dist << 20 | position), one entry fewer is not; a query list may
    // be that long.  The walk reads no list entries.
    std::snprintf(g_where, sizeof g_where, "merge walk limit");
    const int node[2] = {3, 9}, short_begin[3] = {2, 3, 5}, long_begin[3] = {0, 4, 4 + (1 << 20)}, ok_begin[3] = {0, 4, 3 + (1 << 20)};
    int chunks = 1, visits = 0;
    auto count = [&](int, int, int, int) { visits++; };
    CHECK(!for_each_common_node(FeatVec{2, node, short_begin, nullptr}, FeatVec{2, node, long_begin, nullptr}, chunks, count));
    CHECK(visits == 1);   // (the walk ends at the node it refuses)
    CHECK(for_each_common_node(FeatVec{2, node, short_begin, nullptr}, FeatVec{2, node, ok_begin, nullptr}, chunks, count));
    CHECK(chunks == (1 << 20) / 64 && visits == 3);
    CHECK(for_each_common_node(FeatVec{2, node, long_begin, nullptr}, FeatVec{2, node, short_begin, nullptr}, chunks, count) && visits == 5);
    for (const Share* s : {&s_empty_list, &s_begin0, &s_one_empty, &s_disjoint, &s_chunks}) s->print_and_check();
}

// ---------------------------------------------------------------------------------------------------------- rotation filter
struct RotEntry { int slot; float a, b; };
struct RotStats { bool tie34 = false, dropped = false, wrap30 = false, outside = false; };

// the reference's form: 30 vectors in visiting order, ComputeThreeMaxima over them, every other bin's entries withdrawn
static int restated_filter(const std::vector<RotEntry>& e, const std::vector<int>& order, std::vector<int>& out, RotStats& st) {
    const int HISTO_LENGTH = 30;
    std::vector<int> rotHist[HISTO_LENGTH];
    const float factor = 1.0f / HISTO_LENGTH;
    int nmatches = 0;
    for (int k : order) {
        nmatches++;
        float rot = e[k].a - e[k].b;
        if (rot < 0.0) rot += 360.0f;
        int bin = std::isnan(rot) ? -1 : (int)std::round(rot * factor);   // (the drawn angles are NaN or small: the conversion is defined)
        if (bin == HISTO_LENGTH) { bin = 0; st.wrap30 = true; }
        if (!(bin >= 0 && bin < HISTO_LENGTH)) {   // the reference's assert would fire: the match is withdrawn
            out[e[k].slot] = -1; nmatches--; st.outside = true;
            continue;
        }
        rotHist[bin].push_back(e[k].slot);
    }
    int ind1 = -1, ind2 = -1, ind3 = -1;
    {   // ComputeThreeMaxima(rotHist, HISTO_LENGTH, ind1, ind2, ind3)
        int max1 = 0, max2 = 0, max3 = 0;
        for (int i = 0; i < HISTO_LENGTH; i++) {
            const int s = (int)rotHist[i].size();
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
            else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
            else if (s > max3) { max3 = s; ind3 = i; }
        }
        const int before2 = ind2, before3 = ind3;
        if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
        else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
        st.dropped = (before2 >= 0 && ind2 < 0) || (before3 >= 0 && ind3 < 0);
    }
    std::vector<int> sizes;
    for (const std::vector<int>& h : rotHist) sizes.push_back((int)h.size());
    std::sort(sizes.rbegin(), sizes.rend());
    st.tie34 = sizes[3] > 0 && sizes[2] == sizes[3];
    for (int i = 0; i < HISTO_LENGTH; i++) {
        if (i == ind1 || i == ind2 || i == ind3) continue;
        for (size_t j = 0, jend = rotHist[i].size(); j < jend; j++) { out[rotHist[i][j]] = -1; nmatches--; }
    }
    return nmatches;
}

static void test_rotation_filter() {
    Share s_rig{"rotation filter: rig-shaped input (two entries per feature)"}, s_tie{"rotation filter: third and fourth fullest bin tie"},
        s_drop{"rotation filter: second / third maximum dropped by 0.1 * max"}, s_wrap{"rotation filter: a difference that rounds to bin 30"},
        s_nan{"rotation filter: NaN / out-of-range angle (bin -1)"};
    Rng g{23};
    const int scenes = 4000;
    const float kNaN = std::numeric_limits<float>::quiet_NaN();
    for (int sc = 0; sc < scenes; sc++) {
        std::snprintf(g_where, sizeof g_where, "rotation scene %d", sc);
        const bool rig = sc % 2 == 1, concentrated = sc % 4 >= 2, wild = sc % 5 == 0, broken = sc % 5 == 1 || sc % 7 == 0;
        const int per = rig ? 2 : 1, n = 3 + g.below(38), n_slots = per * n + 3;
        // entry k = per * feature + side; for a rig the two entries of a feature point at different slots (left / right frame features)
        std::vector<int> slot_of(per * n, -1), free_slots(n_slots);
        for (int i = 0; i < n_slots; i++) free_slots[i] = i;
        for (int i = n_slots - 1; i > 0; i--) std::swap(free_slots[i], free_slots[g.below(i + 1)]);
        std::vector<float> a(per * n, 0.f), b(per * n, 0.f);
        const float turn = 12.0f * g.below(30);
        for (int k = 0; k < per * n; k++) {
            if (!g.chance(rig ? 0.6f : 0.85f)) continue;
            slot_of[k] = free_slots[k];
            b[k] = 10.0f * g.below(36);
            a[k] = concentrated && !g.chance(0.12f) ? std::fmod(b[k] + turn + (float)(g.below(5) - 2), 360.0f) : 10.0f * g.below(36);
            if (wild && g.chance(0.2f)) { a[k] = 890.0f + 5.0f * g.below(5); b[k] = (float)g.below(4); }   // rot 886 .. 910: bin 30
            if (broken && g.chance(0.15f)) { if (g.chance(0.5f)) a[k] = kNaN; else if (g.chance(0.5f)) b[k] = kNaN; else a[k] = 1500.0f; }
        }
        std::vector<RotEntry> present;
        for (int k = 0; k < per * n; k++) if (slot_of[k] >= 0) present.push_back({slot_of[k], a[k], b[k]});
        std::vector<int> order(present.size());
        for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
        if (sc % 3) for (int i = (int)order.size() - 1; i > 0; i--) std::swap(order[i], order[g.below(i + 1)]);   // (else: the filter's own order)
        std::vector<int> want(n_slots, -1), got(n_slots, -1);
        for (const RotEntry& e : present) want[e.slot] = got[e.slot] = 100 + e.slot;
        for (int check = 1; check >= 0; check--) {
            RotStats st;
            std::vector<int> w = want, o = got;
            const int nw = check ? restated_filter(present, order, w, st) : (int)present.size();
            const int no = rotation_filter(per * n, check, o.data(), [&](int k) { return slot_of[k]; },
                                           [&](int k, float& x, float& y) { CHECK(check); x = a[k]; y = b[k]; });
            CHECK(nw == no);
            CHECK(w == o);
            CHECK(no == (int)std::count_if(o.begin(), o.end(), [](int v) { return v >= 0; }));
            if (check) {
                s_rig.hits += rig; s_tie.hits += st.tie34; s_drop.hits += st.dropped; s_wrap.hits += st.wrap30; s_nan.hits += st.outside;
                for (Share* s : {&s_rig, &s_tie, &s_drop, &s_wrap, &s_nan}) s->scenes++;
            }
        }
    }
    for (const Share* s : {&s_rig, &s_tie, &s_drop, &s_wrap, &s_nan}) s->print_and_check();
}

// ----------------------------------------------------------------------------------------------------------- candidate pick
static void test_candidate_pick() {
    Share s_equal{"candidate pick: equal distances inside a query (last wins)"}, s_claimed{"candidate pick: the best candidate already claimed"},
        s_refused{"candidate pick: the best unclaimed candidate refused"};
    Rng g{37};
    const int scenes = 3000, TH_LOW = 50;
    int q_equal = 0, q_claimed = 0, q_refused = 0, q_all = 0;
    for (int sc = 0; sc < scenes; sc++) {
        std::snprintf(g_where, sizeof g_where, "pick scene %d", sc);
        const int n1 = 1 + g.below(30), n2 = 1 + g.below(40), n_nodes = 1 + g.below(4);
        std::vector<std::vector<int>> q_of(n_nodes), t_of(n_nodes);   // a feature sits in one node; list order drawn
        for (int i = 0; i < n1; i++) q_of[g.below(n_nodes)].push_back(i);
        for (int j = 0; j < n2; j++) t_of[g.below(n_nodes)].push_back(j);
        for (auto* lists : {&q_of, &t_of})
            for (auto& l : *lists) for (int i = (int)l.size() - 1; i > 0; i--) std::swap(l[i], l[g.below(i + 1)]);
        std::vector<int> dist((size_t)n1 * n2);
        for (int& d : dist) d = 10 * (1 + g.below(8));   // eight values, five of them within TH_LOW
        std::vector<uint8_t> ok((size_t)n1 * n2), claimed0(n2);
        for (uint8_t& v : ok) v = g.chance(0.7f);
        for (uint8_t& v : claimed0) v = g.chance(0.4f);
        // the device's list: per node, per query in list order, the trains within TH_LOW in list order
        std::vector<NodeCand> cand;
        for (int nd = 0; nd < n_nodes; nd++)
            for (int i1 : q_of[nd])
                for (size_t p = 0; p < t_of[nd].size(); p++)
                    if (dist[(size_t)i1 * n2 + t_of[nd][p]] <= TH_LOW) cand.push_back({i1, t_of[nd][p], dist[(size_t)i1 * n2 + t_of[nd][p]], (int)p});
        // the reference's scan
        std::vector<int> vMatches12(n1, -1);
        std::vector<uint8_t> vbMatched2 = claimed0;
        for (int nd = 0; nd < n_nodes; nd++)
            for (size_t i1 = 0; i1 < q_of[nd].size(); i1++) {
                const int idx1 = q_of[nd][i1];
                int bestDist = TH_LOW, bestIdx2 = -1;
                int lowest = 1 << 30, lowest_free = 1 << 30, n_lowest_free = 0;   // (coverage only)
                bool lowest_free_refused = false;
                for (size_t i2 = 0; i2 < t_of[nd].size(); i2++) {
                    const int idx2 = t_of[nd][i2], d = dist[(size_t)idx1 * n2 + idx2];
                    if (d <= TH_LOW) lowest = std::min(lowest, d);
                    if (d <= TH_LOW && !vbMatched2[idx2]) {
                        if (d < lowest_free) { lowest_free = d; n_lowest_free = 0; lowest_free_refused = false; }
                        if (d == lowest_free) { n_lowest_free++; lowest_free_refused = !ok[(size_t)idx1 * n2 + idx2]; }
                    }
                    if (vbMatched2[idx2]) continue;
                    if (d > TH_LOW || d > bestDist) continue;
                    if (ok[(size_t)idx1 * n2 + idx2]) { bestIdx2 = idx2; bestDist = d; }
                }
                if (bestIdx2 >= 0) { vMatches12[idx1] = bestIdx2; vbMatched2[bestIdx2] = 1; }
                q_all++; q_equal += n_lowest_free > 1; q_claimed += lowest < lowest_free; q_refused += lowest_free_refused;
            }
        std::vector<int> match12(n1, -1);
        std::vector<uint8_t> claimed = claimed0;
        pick_candidates(cand.data(), cand.size(), claimed.data(), match12.data(), [&](int i1, int i2) { return ok[(size_t)i1 * n2 + i2] != 0; });
        CHECK(match12 == vMatches12);
        CHECK(claimed == vbMatched2);
    }
    s_equal.hits = q_equal; s_claimed.hits = q_claimed; s_refused.hits = q_refused;
    s_equal.scenes = s_claimed.scenes = s_refused.scenes = q_all;   // shares of the queries
    for (const Share* s : {&s_equal, &s_claimed, &s_refused}) s->print_and_check();
}

// ---------------------------------------------------------------------------------------------- camera split, packing
static void test_camera_split() {
    Rng g{41};
    int empty_halves = 0;
    for (int sc = 0; sc < 500; sc++) {
        std::snprintf(g_where, sizeof g_where, "split scene %d", sc);
        const int n = g.below(60), n_left = sc % 7 == 0 ? 0 : sc % 7 == 1 ? n : g.below(n + 1);
        std::vector<int> perm(n);
        for (int i = 0; i < n; i++) perm[i] = i;
        for (int i = n - 1; i > 0; i--) std::swap(perm[i], perm[g.below(i + 1)]);
        Vec v;
        const int begin0 = g.below(3);
        v.begin.push_back(begin0);
        v.feat.assign(begin0, -7);
        for (int used = 0, id = 5; used < n || g.chance(0.3f); id += 1 + g.below(3)) {
            const int l = std::min(n - used, g.below(5));
            v.node.push_back(id);
            v.feat.insert(v.feat.end(), perm.begin() + used, perm.begin() + used + l);
            v.begin.push_back((int)v.feat.size());
            used += l;
        }
        const CameraSplit s = split_by_camera(v.view(), n_left);
        for (int side = 0; side < 2; side++) {
            const OwnedFeatVec& h = side ? s.right : s.left;
            std::vector<int> node, begin{0}, feat;
            for (size_t r = 0; r < v.node.size(); r++) {
                std::vector<int> keep;
                for (int k = v.begin[r]; k < v.begin[r + 1]; k++) if ((v.feat[k] >= n_left) == (side == 1)) keep.push_back(v.feat[k]);
                if (keep.empty()) { empty_halves++; continue; }
                node.push_back(v.node[r]);
                feat.insert(feat.end(), keep.begin(), keep.end());
                begin.push_back((int)feat.size());
            }
            CHECK(h.node == node && h.begin == begin && h.feat == feat);
            const FeatVec view = h.view();
            CHECK(view.nodes == (int)node.size() && view.begin[view.nodes] == (int)feat.size());
            std::vector<uint8_t> seen;
            CHECK(check_feature_vector(n, view, seen));
        }
    }
    CHECK(empty_halves > 500);
}

static void test_packing() {
    Rng g{43};
    for (int sc = 0; sc < 200; sc++) {
        std::snprintf(g_where, sizeof g_where, "packing scene %d", sc);
        const int n = g.below(50), n_levels = 1 + g.below(8);
        std::vector<msorb_keypoint> kp(n);
        std::vector<uint8_t> on(n), stereo(n);
        std::vector<float> scale(n_levels), sigma2(n_levels);
        for (int l = 0; l < n_levels; l++) { scale[l] = 1.0f + 0.37f * l + g.unit(); sigma2[l] = scale[l] * scale[l]; }
        for (int i = 0; i < n; i++) {
            kp[i] = msorb_keypoint{1241 * g.unit(), 376 * g.unit(), 31.f, 360 * g.unit(), 50.f, g.below(n_levels), -1};
            on[i] = (uint8_t)(g.chance(0.3f) ? 0 : 1 + g.below(255));
            stereo[i] = (uint8_t)(g.chance(0.5f) ? 0 : 1 + g.below(255));
        }
        // the loops of the per-call entry: set 1 and set 2
        std::vector<float> xy(2 * n + 1, -1.f), tr(4 * n + 1, -1.f), xy_w = xy, tr_w = tr;
        std::vector<uint8_t> f(n + 1, 9), f_w = f;
        for (int i = 0; i < n; i++) {
            xy_w[2 * i] = kp[i].x;
            xy_w[2 * i + 1] = kp[i].y;
            f_w[i] = (uint8_t)((on[i] ? 1 : 0) | (stereo[i] ? 2 : 0));
        }
        for (int j = 0; j < n; j++) {
            const int oct = kp[j].octave;
            tr_w[4 * j] = kp[j].x;
            tr_w[4 * j + 1] = kp[j].y;
            tr_w[4 * j + 2] = 100 * scale[oct];
            tr_w[4 * j + 3] = sigma2[oct];
        }
        pack_triangulation_side(n, kp.data(), nullptr, nullptr, on.data(), stereo.data(), xy.data(), nullptr, f.data());
        CHECK(xy == xy_w && f == f_w);
        std::fill(f.begin(), f.end(), 9);
        pack_triangulation_side(n, kp.data(), scale.data(), sigma2.data(), on.data(), stereo.data(), nullptr, tr.data(), f.data());
        CHECK(tr == tr_w && f == f_w);
        // the loop of the KeyFrame store: both position forms, no flags
        std::fill(xy.begin(), xy.end(), -1.f); std::fill(tr.begin(), tr.end(), -1.f);
        pack_triangulation_side(n, kp.data(), scale.data(), sigma2.data(), nullptr, nullptr, xy.data(), tr.data(), nullptr);
        CHECK(xy == xy_w && tr == tr_w);
        // flags alone (resident searches): no keypoints at hand
        std::fill(f.begin(), f.end(), 9);
        pack_triangulation_side(n, nullptr, nullptr, nullptr, on.data(), stereo.data(), nullptr, nullptr, f.data());
        CHECK(f == f_w);
    }
}

int main() {
    test_merge_walk();
    test_rotation_filter();
    test_candidate_pick();
    test_camera_split();
    test_packing();
    std::printf("ok\n");
    return 0;
}
