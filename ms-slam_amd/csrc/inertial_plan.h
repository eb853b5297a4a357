// The structure of Optimizer::InertialOptimization's graph (src/Optimizer.cc:3142-3182): one EdgeInertialGS per consecutive
// KeyFrame pair (mPrevKF, KeyFrame).  The device solve needs the velocities in chain order, so that H's velocity part is
// block-tridiagonal: this file checks that the edges form chains and lays the rows out, several chains back to back.  Host only,
// no HIP: tests/inertial_opt_main.cc reads it as it is.
#pragma once
#include <vector>

namespace msorb {
namespace inertial {

struct Plan {
    // Row r of the velocity system is KeyFrame row_kf[r]; e_prev[r] is the edge whose cur it is (-1: a chain starts here),
    // e_next[r] the edge whose prev it is (-1: a chain ends here).  e_next[r] >= 0 joins rows r and r + 1.
    std::vector<int> row_kf, e_prev, e_next;
};

enum PlanError { kPlanOk = 0, kPlanIndex = 1, kPlanFork = 2, kPlanCycle = 3 };

// prev / cur: the KeyFrames of edge e.  A KeyFrame without an edge gets no row (g2o's active set: sparse_optimizer.cpp
// initializeOptimization only takes vertices that an active edge reaches).  Chains come in the order of their first KeyFrame.
inline PlanError make_plan(int n_kf, int n_edges, const int* prev, const int* cur, Plan& plan) {
    plan = Plan();
    if (n_kf < 0 || n_edges < 0) return kPlanIndex;
    std::vector<int> in(n_kf, -1), out(n_kf, -1);
    for (int e = 0; e < n_edges; e++) {
        if (prev[e] < 0 || prev[e] >= n_kf || cur[e] < 0 || cur[e] >= n_kf || prev[e] == cur[e]) return kPlanIndex;
        if (out[prev[e]] >= 0 || in[cur[e]] >= 0) return kPlanFork;
        out[prev[e]] = e;
        in[cur[e]] = e;
    }
    for (int k = 0; k < n_kf; k++) {
        if (in[k] >= 0 || out[k] < 0) continue;           // a chain starts at a KeyFrame with an outgoing edge and no incoming one
        for (int at = k;;) {
            plan.row_kf.push_back(at);
            plan.e_prev.push_back(in[at]);
            plan.e_next.push_back(out[at]);
            if (out[at] < 0) break;
            at = cur[out[at]];
        }
    }
    int with_edge = 0;
    for (int k = 0; k < n_kf; k++) with_edge += (in[k] >= 0 || out[k] >= 0) ? 1 : 0;
    if ((int)plan.row_kf.size() != with_edge) { plan = Plan(); return kPlanCycle; }   // what no chain start reaches is on a cycle
    return kPlanOk;
}

}  // namespace inertial
}  // namespace msorb
