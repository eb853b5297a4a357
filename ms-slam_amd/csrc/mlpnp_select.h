// The sequential part of MLPnPsolver::iterate (src/MLPnPsolver.cpp:212-245 and :248-263) over the inlier counts of hypotheses that
// were all evaluated beforehand: which hypothesis the loop would have ended on.  One statement for the device (mlpnp_select_kernel,
// mlpnp.hip), the host replay of the chunks (host/MLPnPsolver_device.h) and the host test (tests/mlpnp_main.cc).
//
// The rule is not Sim3Solver's (sim3_select.h).  Under count >= min_inliers (:212) a hypothesis replaces the running best only when
// count > best (:215, ties stay with the earlier one), and Refine() (:232, :338-396) then returns true whenever count > min_inliers
// (:379), whether or not the hypothesis became the best: Refine's own computePose goes into a local that nothing reads, and the
// CheckInliers behind it counts the CURRENT hypothesis again.  So the loop ends on the first count > min_inliers and hands out that
// hypothesis; at exhaustion (:248-263) it hands out the best.
#pragma once

#if defined(__HIPCC__)
#define MLPNP_SEL_HD __host__ __device__ inline
#else
#define MLPNP_SEL_HD inline
#endif

namespace msorb {

struct MlpnpSelection {
    int winner;      // converged: the hypothesis the loop returned at; otherwise best_h
    int converged;   // the loop returned true at `winner` from Refine() (:232-243)
    int consumed;    // iterations the loop went through (mnIterations advances by this): winner + 1 when converged, n otherwise
    int best;        // mnBestInliers afterwards
    int best_h;      // the last hypothesis that raised the best (whose mask / pose mvbBestInliers / mBestTcw hold); -1: none did
};

// counts[0, n) in hypothesis order; best_in = mnBestInliers before the loop.
MLPNP_SEL_HD MlpnpSelection mlpnp_select(const int* counts, int n, int min_inliers, int best_in) {
    MlpnpSelection r{-1, 0, n < 0 ? 0 : n, best_in, -1};
    for (int i = 0; i < n; i++) {
        const int c = counts[i];
        if (c >= min_inliers) {
            if (c > r.best) {
                r.best = c;
                r.best_h = i;
            }
            if (c > min_inliers) {
                r.winner = i;
                r.converged = 1;
                r.consumed = i + 1;
                return r;
            }
        }
    }
    r.winner = r.best_h;
    return r;
}

// The rule is a fold, so a long vector can be taken in pieces: `sel` is the state after counts[0, base) (start it as
// {-1, 0, n_total, best_in, -1}), chunk[0, m) are counts[base, base + m).  Nothing changes once sel.converged is set.
MLPNP_SEL_HD void mlpnp_select_continue(MlpnpSelection& sel, const int* chunk, int m, int base, int min_inliers) {
    if (sel.converged) return;
    const MlpnpSelection c = mlpnp_select(chunk, m, min_inliers, sel.best);
    if (c.best_h >= 0) { sel.best_h = base + c.best_h; sel.best = c.best; }
    if (c.converged) { sel.converged = 1; sel.winner = base + c.winner; sel.consumed = base + c.consumed; }
    else sel.winner = sel.best_h;
}

}  // namespace msorb
