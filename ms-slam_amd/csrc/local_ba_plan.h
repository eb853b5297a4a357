// The index lists of one bundle adjustment, local or global (bundle_adjustment.hip), built once per call on the host.  Host only: no HIP, no library,
// so tests/local_ba_plan_main.cc checks it against a brute-force enumeration without a device (and under the sanitizers).
//
// Edges arrive point-major (point 0's edges, then point 1's, ...: Optimizer.cc:1196-1320 builds them that way), so the by-point
// CSR is the run boundaries of edge_point.  Every sum of the solver walks one of these lists in ascending position, which is what
// makes a result independent of how the device schedules it:
//   point_begin [P + 1]        edges of point p = [point_begin[p], point_begin[p + 1])
//   free_of_kf  [K]            the KeyFrame's block index in the reduced system (its rank among the free KeyFrames), -1 = fixed
//   kf_of_free  [Kf]
//   kf_begin    [Kf + 1], kf_edge      the edges of free KeyFrame i, ascending edge index
//   pair_i, pair_j [NP], pair_begin [NP + 1], pair_a, pair_b
//                              the block (i, j), i <= j, of the reduced system receives  - W_a D^-1 W_b^T  for every listed (a, b):
//                              edges of ONE point with free(a) = i, free(b) = j.  Pairs are sorted by (i, j); inside a pair the
//                              entries keep the order of the points (ascending a, then b), which is the order in which g2o's loop
//                              over the landmarks subtracts them (block_solver.hpp:381-432).  (i, i) is listed for every free
//                              KeyFrame, also with no entry (its block is then Hpp + lambda I alone).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace msorb {

struct LocalBaPlan {
    int K = 0, Kf = 0, P = 0, E = 0;
    std::vector<int> point_begin, free_of_kf, kf_of_free, kf_begin, kf_edge, pair_i, pair_j, pair_begin, pair_a, pair_b;
    size_t longest_point = 0;   // edges of the point with the most
};

enum LocalBaPlanError { kPlanOk = 0, kPlanIndexOutOfRange = 1, kPlanNotPointMajor = 2 };

// kf_fixed [K] (non-zero = fixed), edge_kf / edge_point [E].  Nothing of `plan` is meaningful unless kPlanOk is returned.
inline LocalBaPlanError build_local_ba_plan(int K, const int* kf_fixed, int P, int E, const int* edge_kf, const int* edge_point,
                                            LocalBaPlan& plan) {
    plan = LocalBaPlan();
    plan.K = K; plan.P = P; plan.E = E;
    for (int e = 0; e < E; e++) {
        if (edge_kf[e] < 0 || edge_kf[e] >= K || edge_point[e] < 0 || edge_point[e] >= P) return kPlanIndexOutOfRange;
        if (e > 0 && edge_point[e] < edge_point[e - 1]) return kPlanNotPointMajor;
    }
    plan.free_of_kf.assign((size_t)K, -1);
    for (int k = 0; k < K; k++)
        if (!kf_fixed[k]) { plan.free_of_kf[k] = plan.Kf++; plan.kf_of_free.push_back(k); }
    const int Kf = plan.Kf;
    plan.point_begin.assign((size_t)P + 1, 0);
    for (int e = 0; e < E; e++) plan.point_begin[(size_t)edge_point[e] + 1]++;
    for (int p = 0; p < P; p++) {
        plan.longest_point = std::max(plan.longest_point, (size_t)plan.point_begin[(size_t)p + 1]);
        plan.point_begin[(size_t)p + 1] += plan.point_begin[p];
    }
    // by free KeyFrame: a counting sort, which keeps the edges ascending
    plan.kf_begin.assign((size_t)Kf + 1, 0);
    for (int e = 0; e < E; e++) {
        const int i = plan.free_of_kf[edge_kf[e]];
        if (i >= 0) plan.kf_begin[(size_t)i + 1]++;
    }
    for (int i = 0; i < Kf; i++) plan.kf_begin[(size_t)i + 1] += plan.kf_begin[i];
    plan.kf_edge.resize((size_t)plan.kf_begin[Kf]);
    {
        std::vector<int> at(plan.kf_begin.begin(), plan.kf_begin.end() - 1);
        for (int e = 0; e < E; e++) {
            const int i = plan.free_of_kf[edge_kf[e]];
            if (i >= 0) plan.kf_edge[(size_t)at[i]++] = e;
        }
    }
    // block pairs: every (a, b) of one point with free(a) <= free(b); two edges of one point on the SAME KeyFrame (the reference
    // never makes them: its observations are a map keyed by KeyFrame) would contribute both (a, b) and (b, a) to (i, i)
    struct Entry { int64_t key; int a, b; };
    std::vector<Entry> entries;
    for (int p = 0; p < P; p++)
        for (int a = plan.point_begin[p]; a < plan.point_begin[(size_t)p + 1]; a++) {
            const int i = plan.free_of_kf[edge_kf[a]];
            if (i < 0) continue;
            for (int b = plan.point_begin[p]; b < plan.point_begin[(size_t)p + 1]; b++) {
                const int j = plan.free_of_kf[edge_kf[b]];
                if (j < i) continue;
                entries.push_back(Entry{(int64_t)i * Kf + j, a, b});
            }
        }
    std::stable_sort(entries.begin(), entries.end(), [](const Entry& x, const Entry& y) { return x.key < y.key; });
    plan.pair_begin.push_back(0);
    size_t at = 0;
    for (int i = 0; i < Kf; i++) {   // (i, i) first, always; then the (i, j > i) that have entries
        int64_t open = (int64_t)i * Kf + i;
        plan.pair_i.push_back(i);
        plan.pair_j.push_back(i);
        for (; at < entries.size() && entries[at].key / Kf == i; at++) {
            if (entries[at].key != open) {
                plan.pair_begin.push_back((int)plan.pair_a.size());
                open = entries[at].key;
                plan.pair_i.push_back(i);
                plan.pair_j.push_back((int)(open % Kf));
            }
            plan.pair_a.push_back(entries[at].a);
            plan.pair_b.push_back(entries[at].b);
        }
        plan.pair_begin.push_back((int)plan.pair_a.size());
    }
    return kPlanOk;
}

}  // namespace msorb
