// The three sequential rules of TwoViewReconstruction (src/TwoViewReconstruction.cc), one statement for the kernels, the host part of
// msorb_two_view_reconstruct and the host program of the tests:
//   tv_fold_continue   the fold of FindHomography / FindFundamental (:172-177, :223-228) over the scores in hypothesis order
//   tv_branch          Reconstruct's choice between the two models (:113-128)
//   tv_final_f / _h    the closing rules of ReconstructF (:505-568) and ReconstructH (:693-733) over the records (nGood, parallax)
// The comparisons against 0.7 * maxGood, 0.75 * bestGood, 0.9 * N are double as the reference's expressions are.
#pragma once
#include "new_points_device.h"

namespace msorb {

enum TvBranch : int { kTvNoModel = 0, kTvHomography = 1, kTvFundamental = 2 };

struct TvFold {
    float score;   // starts at 0 (:144, :195)
    int winner;    // -1: no hypothesis exceeded 0, the model and the mask stay as the caller left them
};

// `currentScore > score` over s[0..n), hypothesis i of the chunk being base + i.  A NaN score is not greater and never wins.
NP_HD void tv_fold_continue(TvFold& f, const float* s, int n, int base) {
    for (int i = 0; i < n; i++)
        if (s[i] > f.score) { f.score = s[i]; f.winner = base + i; }
}

// :113-128.  h_ratio is the reference's 0.50 (a double literal: the float RH is widened for the comparison).
NP_HD int tv_branch(float SH, float SF, double h_ratio, float& RH) {
    const float sum = np_add(SH, SF);
    RH = 0.0f;
    if (sum == 0.0f) return kTvNoModel;
    RH = np_div(SH, sum);
    return (double)RH > h_ratio ? kTvHomography : kTvFundamental;
}

// static_cast<int>(0.9 * N) against minTriangulated (:507)
NP_HD int tv_min_good(int n_inliers, int min_triangulated) {
    const int a = (int)np_dmul(0.9, (double)n_inliers);
    return a > min_triangulated ? a : min_triangulated;
}

// :505-568: the index of the motion hypothesis that is handed out, -1 for `return false`.
NP_HD int tv_final_f(const int* n_good, const float* parallax, int n_inliers, float min_parallax, int min_triangulated) {
    int max_good = n_good[0];
    for (int i = 1; i < 4; i++) max_good = n_good[i] > max_good ? n_good[i] : max_good;   // max(a, max(b, max(c, d))): the same integer
    const int n_min_good = tv_min_good(n_inliers, min_triangulated);
    const double lim = np_dmul(0.7, (double)max_good);
    int nsimilar = 0;
    for (int i = 0; i < 4; i++)
        if ((double)n_good[i] > lim) nsimilar++;
    if (max_good < n_min_good || nsimilar > 1) return -1;
    for (int i = 0; i < 4; i++)   // the else-if chain: the first hypothesis that holds the maximum decides alone
        if (max_good == n_good[i]) return parallax[i] > min_parallax ? i : -1;
    return -1;
}

// :693-733
NP_HD int tv_final_h(const int* n_good, const float* parallax, int n_inliers, float min_parallax, int min_triangulated) {
    int best = 0, second = 0, idx = -1;
    float best_parallax = -1.0f;
    for (int i = 0; i < 8; i++) {
        if (n_good[i] > best) {
            second = best;
            best = n_good[i];
            idx = i;
            best_parallax = parallax[i];
        } else if (n_good[i] > second) {
            second = n_good[i];
        }
    }
    if ((double)second < np_dmul(0.75, (double)best) && best_parallax >= min_parallax && best > min_triangulated &&
        (double)best > np_dmul(0.9, (double)n_inliers))
        return idx;
    return -1;
}

}  // namespace msorb
