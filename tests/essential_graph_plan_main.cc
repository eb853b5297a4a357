// ms-slam_amd/csrc/essential_graph_plan.h (the index lists of the device's essential-graph optimisation) against a brute-force enumeration.
//
//   essential_graph_plan in.bin
// in : N E (int) | fixed[N] | v0[E] | v1[E] (int)
// Prints one line of sizes and "ok"; any mismatch prints what differs and exits with 1.  Then the two refusals: an index out of
// range and an edge from a vertex to itself.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../ms-slam_amd/csrc/essential_graph_plan.h"

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
    int dims[2];
    if (std::fread(dims, 4, 2, in) != 2) return 2;
    const int N = dims[0], E = dims[1];
    std::vector<int> fixed(N), v0(E), v1(E);
    if (std::fread(fixed.data(), 4, N, in) != (size_t)N || std::fread(v0.data(), 4, E, in) != (size_t)E ||
        std::fread(v1.data(), 4, E, in) != (size_t)E)
        return 2;
    std::fclose(in);
    msorb::EssentialGraphPlan pl;
    CHECK(msorb::build_essential_graph_plan(N, fixed.data(), E, v0.data(), v1.data(), pl) == msorb::kEgPlanOk);
    // the active edges, and the free vertices that have one, in input order
    std::vector<int> active;
    std::vector<char> used(N, 0);
    for (int e = 0; e < E; e++) {
        if (fixed[v0[e]] && fixed[v1[e]]) continue;
        active.push_back(e);
        used[v0[e]] = used[v1[e]] = 1;
    }
    CHECK(pl.Ea == (int)active.size() && pl.active_edge == active);
    int Kf = 0;
    for (int k = 0; k < N; k++) {
        if (fixed[k] || !used[k]) { CHECK(pl.free_of_vertex[k] == -1); continue; }
        CHECK(pl.free_of_vertex[k] == Kf && pl.vertex_of_free[Kf] == k);
        Kf++;
    }
    CHECK(pl.Kf == Kf && (int)pl.vertex_of_free.size() == Kf);
    // incident lists: brute force over all active edges
    CHECK((int)pl.inc_begin.size() == Kf + 1 && pl.inc_begin[0] == 0);
    size_t longest = 0;
    for (int i = 0; i < Kf; i++) {
        std::vector<int> want;
        for (int a = 0; a < pl.Ea; a++) {
            if (v0[active[a]] == pl.vertex_of_free[i]) want.push_back(2 * a);
            if (v1[active[a]] == pl.vertex_of_free[i]) want.push_back(2 * a + 1);
        }
        CHECK(pl.inc_begin[i + 1] - pl.inc_begin[i] == (int)want.size());
        for (size_t m = 0; m < want.size(); m++) CHECK(pl.inc_entry[pl.inc_begin[i] + m] == want[m]);
        longest = std::max(longest, want.size());
    }
    CHECK((size_t)pl.inc_begin[Kf] == pl.inc_entry.size());
    // pairs: brute force
    std::map<std::pair<int, int>, std::vector<int>> want;
    for (int a = 0; a < pl.Ea; a++) {
        const int i = pl.free_of_vertex[v0[active[a]]], j = pl.free_of_vertex[v1[active[a]]];
        if (i < 0 || j < 0) continue;
        if (i < j) want[{i, j}].push_back(2 * a);
        else want[{j, i}].push_back(2 * a + 1);
    }
    const size_t NP = pl.pair_i.size();
    CHECK(NP == want.size() && pl.pair_j.size() == NP && pl.pair_begin.size() == NP + 1 && pl.pair_begin[0] == 0);
    size_t q = 0, entries = 0, longest_pair = 0;
    for (const auto& kv : want) {   // (the map walks (i, j) ascending: the plan's order)
        CHECK(pl.pair_i[q] == kv.first.first && pl.pair_j[q] == kv.first.second && pl.pair_i[q] < pl.pair_j[q]);
        CHECK(pl.pair_begin[q + 1] - pl.pair_begin[q] == (int)kv.second.size());
        for (size_t m = 0; m < kv.second.size(); m++) CHECK(pl.pair_entry[pl.pair_begin[q] + m] == kv.second[m]);
        entries += kv.second.size();
        longest_pair = std::max(longest_pair, kv.second.size());
        q++;
    }
    CHECK(entries == pl.pair_entry.size());
    std::printf("N %d free %d E %d active %d longest_incident %zu pairs %zu entries %zu longest_pair %zu\n", N, Kf, E, pl.Ea, longest, NP,
                entries, longest_pair);
    // the refusals
    if (E > 0) {
        msorb::EssentialGraphPlan bad;
        std::vector<int> a = v0, b = v1;
        a[E - 1] = N;
        CHECK(msorb::build_essential_graph_plan(N, fixed.data(), E, a.data(), v1.data(), bad) == msorb::kEgPlanIndexOutOfRange);
        b[0] = -1;
        CHECK(msorb::build_essential_graph_plan(N, fixed.data(), E, v0.data(), b.data(), bad) == msorb::kEgPlanIndexOutOfRange);
        b = v1;
        b[0] = v0[0];
        CHECK(msorb::build_essential_graph_plan(N, fixed.data(), E, v0.data(), b.data(), bad) == msorb::kEgPlanSelfEdge);
    }
    std::printf("ok\n");
    return 0;
}
