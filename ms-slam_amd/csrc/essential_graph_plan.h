// The index lists of one essential-graph optimisation (essential_graph.hip), built once per call on the host.  Host only: no HIP,
// no library, so tests/essential_graph_plan_main.cc checks it against a brute-force enumeration without a device (and under the
// sanitizers).  It sits beside local_ba_plan.h and follows its style: every sum of the solver walks one of these lists in ascending
// position, which is what makes a result independent of how the device schedules it.
//
// g2o's active set (sparse_optimizer.cpp:234): an edge whose two vertices are both fixed is not active; a free vertex without an
// active edge is not in the system.
//   active_edge [Ea]           the caller's index of active edge a, ascending
//   free_of_vertex [N]         the vertex's block index in the system (its rank among the free vertices that have an active edge),
//                              -1 = fixed, or free without an active edge
//   vertex_of_free [Kf]
//   inc_begin [Kf + 1], inc_entry
//                              free vertex i receives H_ii and b_i from every listed entry 2 a + side: active edge a, of which it is
//                              vertex `side` (0: the Jacobian A, 1: B); ascending a
//   pair_i, pair_j [NP], pair_begin [NP + 1], pair_entry
//                              the block (i, j), i < j, receives H_ij from every listed entry 2 a + flip: flip 0, vertex 0 of edge a is
//                              i and the term is A^T B; flip 1, vertex 0 is j and the term is its transpose.  Pairs sorted by (i, j),
//                              entries ascending a: several edges between one pair of KeyFrames are ONE pair with several entries.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace msorb {

struct EssentialGraphPlan {
    int N = 0, Kf = 0, E = 0, Ea = 0;
    std::vector<int> active_edge, free_of_vertex, vertex_of_free, inc_begin, inc_entry, pair_i, pair_j, pair_begin, pair_entry;
};

enum EssentialGraphPlanError { kEgPlanOk = 0, kEgPlanIndexOutOfRange = 1, kEgPlanSelfEdge = 2 };

// fixed [N] (non-zero = fixed), v0 / v1 [E].  Nothing of `plan` is meaningful unless kEgPlanOk is returned.
inline EssentialGraphPlanError build_essential_graph_plan(int N, const int* fixed, int E, const int* v0, const int* v1,
                                                          EssentialGraphPlan& plan) {
    plan = EssentialGraphPlan();
    plan.N = N; plan.E = E;
    for (int e = 0; e < E; e++) {
        if (v0[e] < 0 || v0[e] >= N || v1[e] < 0 || v1[e] >= N) return kEgPlanIndexOutOfRange;
        if (v0[e] == v1[e]) return kEgPlanSelfEdge;
    }
    std::vector<uint8_t> in_system((size_t)N, 0);
    for (int e = 0; e < E; e++) {
        if (fixed[v0[e]] && fixed[v1[e]]) continue;
        plan.active_edge.push_back(e);
        if (!fixed[v0[e]]) in_system[v0[e]] = 1;
        if (!fixed[v1[e]]) in_system[v1[e]] = 1;
    }
    plan.Ea = (int)plan.active_edge.size();
    plan.free_of_vertex.assign((size_t)N, -1);
    for (int k = 0; k < N; k++)
        if (in_system[k]) { plan.free_of_vertex[k] = plan.Kf++; plan.vertex_of_free.push_back(k); }
    const int Kf = plan.Kf, Ea = plan.Ea;
    // by free vertex: a counting sort, which keeps the edges ascending
    plan.inc_begin.assign((size_t)Kf + 1, 0);
    for (int a = 0; a < Ea; a++) {
        const int e = plan.active_edge[a];
        for (int side = 0; side < 2; side++) {
            const int i = plan.free_of_vertex[side ? v1[e] : v0[e]];
            if (i >= 0) plan.inc_begin[(size_t)i + 1]++;
        }
    }
    for (int i = 0; i < Kf; i++) plan.inc_begin[(size_t)i + 1] += plan.inc_begin[i];
    plan.inc_entry.resize((size_t)plan.inc_begin[Kf]);
    {
        std::vector<int> at(plan.inc_begin.begin(), plan.inc_begin.end() - 1);
        for (int a = 0; a < Ea; a++) {
            const int e = plan.active_edge[a];
            for (int side = 0; side < 2; side++) {
                const int i = plan.free_of_vertex[side ? v1[e] : v0[e]];
                if (i >= 0) plan.inc_entry[(size_t)at[i]++] = 2 * a + side;
            }
        }
    }
    // block pairs of the edges with two free ends
    struct Entry { int64_t key; int entry; };
    std::vector<Entry> entries;
    for (int a = 0; a < Ea; a++) {
        const int e = plan.active_edge[a];
        const int i = plan.free_of_vertex[v0[e]], j = plan.free_of_vertex[v1[e]];
        if (i < 0 || j < 0) continue;
        if (i < j) entries.push_back(Entry{(int64_t)i * Kf + j, 2 * a});
        else entries.push_back(Entry{(int64_t)j * Kf + i, 2 * a + 1});
    }
    std::stable_sort(entries.begin(), entries.end(), [](const Entry& x, const Entry& y) { return x.key < y.key; });
    plan.pair_begin.push_back(0);
    for (size_t at = 0; at < entries.size(); at++) {
        if (at == 0 || entries[at].key != entries[at - 1].key) {
            if (at) plan.pair_begin.push_back((int)plan.pair_entry.size());
            plan.pair_i.push_back((int)(entries[at].key / Kf));
            plan.pair_j.push_back((int)(entries[at].key % Kf));
        }
        plan.pair_entry.push_back(entries[at].entry);
    }
    if (!entries.empty()) plan.pair_begin.push_back((int)plan.pair_entry.size());
    return kEgPlanOk;
}

}  // namespace msorb
