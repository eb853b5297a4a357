// The sequential part of Sim3Solver::iterate (src/Sim3Solver.cc:344-366, the same rule at :271-288) over the inlier counts of
// hypotheses that were all evaluated beforehand: which hypothesis the loop would have ended on.  One statement for the device
// (sim3_select_kernel, sim3.hip), the host replay of the chunks (host/Sim3Solver_device.h) and the host test
// (tests/sim3_select_main.cc).
#pragma once

#if defined(__HIPCC__)
#define SIM3_SEL_HD __host__ __device__ inline
#else
#define SIM3_SEL_HD inline
#endif

namespace msorb {

struct Sim3Selection {
    int winner;      // the last hypothesis that replaced the running best; -1: none reached best_in
    int converged;   // the scan stopped at `winner` because its count exceeds min_inliers (:353)
    int consumed;    // hypotheses the loop went through (mnIterations advances by this): winner + 1 when converged, n otherwise
    int best;        // mnBestInliers afterwards
};

// counts[0, n) in hypothesis order; best_in = mnBestInliers before the loop.  A hypothesis replaces the running best when
// count >= best (:344: ties go to the later one); the loop ends at the first one where that holds and count > min_inliers.
SIM3_SEL_HD Sim3Selection sim3_select(const int* counts, int n, int min_inliers, int best_in) {
    Sim3Selection r{-1, 0, n < 0 ? 0 : n, best_in};
    for (int i = 0; i < n; i++) {
        const int c = counts[i];
        if (c >= r.best) {
            r.best = c;
            r.winner = i;
            if (c > min_inliers) {
                r.converged = 1;
                r.consumed = i + 1;
                return r;
            }
        }
    }
    return r;
}

// The rule is a fold, so a long vector can be taken in pieces: `sel` is the state after counts[0, base) (start it as
// {-1, 0, n_total, best_in}), chunk[0, m) are counts[base, base + m).  Nothing changes once sel.converged is set.
SIM3_SEL_HD void sim3_select_continue(Sim3Selection& sel, const int* chunk, int m, int base, int min_inliers) {
    if (sel.converged) return;
    const Sim3Selection c = sim3_select(chunk, m, min_inliers, sel.best);
    if (c.winner >= 0) { sel.winner = base + c.winner; sel.best = c.best; }
    if (c.converged) { sel.converged = 1; sel.consumed = base + c.consumed; }
}

}  // namespace msorb
