// g2o's Levenberg loop as this fork runs it (g2o/core/optimization_algorithm_levenberg.cpp:61-170 under sparse_optimizer.cpp:376-389),
// once, for code that runs INSIDE a kernel and for the host compiler that reads the same header: computeLambdaInit (:172-186: the
// user's value or tau times the largest |H(j, j)|), up to ten trials per iteration, rho against computeScale (:188-195), the
// lambda updates, Terminate on ten rejected trials or rho == 0 (:151-155), and the fork's _nBad stop (:157-167).  The routine states
// the control flow only; the three callables own the state and its two copies (push / pop):
//   linearise(max_diagonal) -> cost     computeActiveErrors + activeRobustChi2 + buildSystem at the estimate
//   trial(lambda, solved, scale) -> cost  setLambda, solve, update(x) into the other copy, the cost there, computeScale's sum;
//                                         solved = false: a pivot that was not positive
//   accept()                            discardTop: the other copy becomes the estimate
// Every executor of a workgroup runs it with equal bits in every argument, so all of them take the same branches.  eg::levenberg
// (essential_graph_device.h) is the same loop for a backend the HOST drives, launch by launch; pose_opt.hip and sim3_opt_device.h,
// written before this header, carry their own copies of the text.
#pragma once
#include <cfloat>
#include <cmath>

#include "se3_device.h"

namespace msorb {
namespace lm {

struct Counts { int iterations, rejected; double chi2_initial; int trials; double lambda; };   // lambda: as the last trial left it

template <typename Linearise, typename Trial, typename Accept>
SE3_HD Counts levenberg(int max_it, bool user_lambda_init, double user_lambda, Linearise linearise, Trial trial, Accept accept) {
    Counts n{0, 0, 0.0, 0, 0.0};
    double lambda = 0, ni = 2;
    int n_bad = 0;
    bool ok = true;
    for (int i = 0; i < max_it && ok; i++) {                                   // sparse_optimizer.cpp:376
        double max_diagonal = 0;
        double current = linearise(max_diagonal), temp = current;
        const double ini = current;
        if (i == 0) {                                                          // :93-97, computeLambdaInit (:172-186), _tau = 1e-5
            n.chi2_initial = current;
            lambda = user_lambda_init ? user_lambda : 1e-5 * max_diagonal;
            ni = 2;
            n_bad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            bool solved = true;
            double scale = 0;
            temp = trial(lambda, solved, scale);                               // :103-124
            if (!solved) temp = DBL_MAX;                                       // :126-127
            rho = current - temp;
            rho /= scale + 1e-3;                                               // :129-131
            if (rho > 0 && isfinite(temp)) {                                   // :134-142
                const double y = 2 * rho - 1;
                double alpha = 1. - (y * y) * y;                               // pow(2 rho - 1, 3)
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2;
                current = temp;
                accept();                                                      // discardTop
            } else {                                                           // :143-147: pop
                lambda *= ni;
                ni *= 2;
                n.rejected++;
            }
            qmax++;
            n.trials++;
        } while (rho < 0 && qmax < 10);                                        // :149
        n.iterations++;
        if (qmax == 10 || rho == 0) { ok = false; continue; }                  // :151-155 Terminate
        if ((ini - current) * 1e3 < ini) n_bad++;                              // :157-162: this fork's _nBad stop
        else n_bad = 0;
        if (n_bad >= 3) ok = false;                                            // :164-167
    }
    n.lambda = lambda;
    return n;
}

}  // namespace lm
}  // namespace msorb
