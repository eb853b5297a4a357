// ms-slam_amd/csrc/local_ba_plan.h (the index lists of the device's local bundle adjustment) against a brute-force enumeration.
//
//   local_ba_plan in.bin
// in : K P E (int) | fixed[K] | edge_kf[E] | edge_point[E] (int)
// Prints one line of sizes and "ok"; any mismatch prints what differs and exits with 1.  Then the two refusals: an index out of
// range and edges that are not point-major.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "local_ba_plan.h"

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("line %d: %s does not hold\n", __LINE__, #c); \
            return 1;                                              \
        }                                                          \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int dims[3];
    if (std::fread(dims, 4, 3, in) != 3) return 2;
    const int K = dims[0], P = dims[1], E = dims[2];
    std::vector<int> fixed(K), ek(E), ep(E);
    if (std::fread(fixed.data(), 4, K, in) != (size_t)K || std::fread(ek.data(), 4, E, in) != (size_t)E ||
        std::fread(ep.data(), 4, E, in) != (size_t)E)
        return 2;
    std::fclose(in);
    msorb::LocalBaPlan pl;
    CHECK(msorb::build_local_ba_plan(K, fixed.data(), P, E, ek.data(), ep.data(), pl) == msorb::kPlanOk);
    // free KeyFrames in input order
    int Kf = 0;
    for (int k = 0; k < K; k++) {
        if (fixed[k]) { CHECK(pl.free_of_kf[k] == -1); continue; }
        CHECK(pl.free_of_kf[k] == Kf && pl.kf_of_free[Kf] == k);
        Kf++;
    }
    CHECK(pl.Kf == Kf && (int)pl.kf_of_free.size() == Kf);
    // by point
    CHECK((int)pl.point_begin.size() == P + 1 && pl.point_begin[0] == 0 && pl.point_begin[P] == E);
    size_t longest = 0;
    for (int p = 0; p < P; p++) {
        for (int e = pl.point_begin[p]; e < pl.point_begin[p + 1]; e++) CHECK(ep[e] == p);
        longest = std::max(longest, (size_t)(pl.point_begin[p + 1] - pl.point_begin[p]));
    }
    CHECK(pl.longest_point == longest);
    // by free KeyFrame: brute force over all edges
    CHECK((int)pl.kf_begin.size() == Kf + 1 && pl.kf_begin[0] == 0);
    for (int i = 0; i < Kf; i++) {
        std::vector<int> want;
        for (int e = 0; e < E; e++)
            if (ek[e] == pl.kf_of_free[i]) want.push_back(e);
        CHECK(pl.kf_begin[i + 1] - pl.kf_begin[i] == (int)want.size());
        for (size_t m = 0; m < want.size(); m++) CHECK(pl.kf_edge[pl.kf_begin[i] + m] == want[m]);
    }
    CHECK((size_t)pl.kf_begin[Kf] == pl.kf_edge.size());
    // block pairs: brute force over all pairs of edges
    std::map<std::pair<int, int>, std::vector<std::pair<int, int>>> want;
    for (int i = 0; i < Kf; i++) want[{i, i}];
    for (int a = 0; a < E; a++)
        for (int b = 0; b < E; b++) {
            if (ep[a] != ep[b] || fixed[ek[a]] || fixed[ek[b]]) continue;
            const int i = pl.free_of_kf[ek[a]], j = pl.free_of_kf[ek[b]];
            if (i <= j) want[{i, j}].push_back({a, b});
        }
    const size_t NP = pl.pair_i.size();
    CHECK(NP == want.size() && pl.pair_j.size() == NP && pl.pair_begin.size() == NP + 1 && pl.pair_begin[0] == 0);
    size_t q = 0, entries = 0, longest_pair = 0;
    for (const auto& kv : want) {   // (the map walks (i, j) ascending: the plan's order)
        CHECK(pl.pair_i[q] == kv.first.first && pl.pair_j[q] == kv.first.second);
        CHECK(pl.pair_begin[q + 1] - pl.pair_begin[q] == (int)kv.second.size());
        for (size_t m = 0; m < kv.second.size(); m++) {
            CHECK(pl.pair_a[pl.pair_begin[q] + m] == kv.second[m].first);
            CHECK(pl.pair_b[pl.pair_begin[q] + m] == kv.second[m].second);
        }
        entries += kv.second.size();
        longest_pair = std::max(longest_pair, kv.second.size());
        q++;
    }
    CHECK(entries == pl.pair_a.size() && entries == pl.pair_b.size());
    std::printf("K %d free %d P %d E %d longest_point %zu pairs %zu entries %zu longest_pair %zu\n", K, Kf, P, E, longest, NP, entries,
                longest_pair);
    // the refusals
    if (E > 1) {
        msorb::LocalBaPlan bad;
        std::vector<int> ek2 = ek, ep2 = ep;
        ek2[E - 1] = K;
        CHECK(msorb::build_local_ba_plan(K, fixed.data(), P, E, ek2.data(), ep.data(), bad) == msorb::kPlanIndexOutOfRange);
        ep2[0] = -1;
        CHECK(msorb::build_local_ba_plan(K, fixed.data(), P, E, ek.data(), ep2.data(), bad) == msorb::kPlanIndexOutOfRange);
        ep2 = ep;
        ep2[0] = P - 1;
        if (ep[1] < P - 1) CHECK(msorb::build_local_ba_plan(K, fixed.data(), P, E, ek.data(), ep2.data(), bad) == msorb::kPlanNotPointMajor);
    }
    std::printf("ok\n");
    return 0;
}
