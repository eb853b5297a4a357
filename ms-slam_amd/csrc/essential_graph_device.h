// Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1410-1675 and :1677-1985) after the gathering loops: g2o's Sim3::log
// (types/sim3.h:148-230), EdgeSim3::computeError (types_seven_dof_expmap.h:106-114), the NUMERIC Jacobian the edge gets from
// BaseBinaryEdge::linearizeOplus (core/base_binary_edge.hpp:131-203; EdgeSim3 has no linearizeOplus of its own), the terms of
// constructQuadraticForm without a kernel (:55-90) and the Levenberg loop (optimization_algorithm_levenberg.cpp:61-170 under
// sparse_optimizer.cpp:376-389, lambda from setUserLambdaInit).  One statement of the arithmetic for the device
// (essential_graph.hip) and the host (tests/essential_graph_main.cc): plain double arithmetic in the order written, nothing
// contracted (-ffp-contract=off).  Sim3, its product, inverse and exponential are sim3_opt_device.h's.  DESIGN.md section 17.
#pragma once
#include <cfloat>
#include <cmath>

#include "sim3_opt_device.h"

namespace msorb {
namespace eg {

using sim3opt::Sim3;
using sim3opt::sim3_exp;
using sim3opt::sim3_inverse;
using sim3opt::sim3_mul;

// planes of the edge-major linearisation: A^T A and B^T B (upper triangles, row major), A^T B (full), A^T (-e), B^T (-e)
constexpr int kHaa = 0, kHbb = 28, kHab = 56, kBa = 105, kBb = 112, kPlanes = 119;
// the error vectors of one linearisation: 0 the base error, 1 + k vertex 0 perturbed by table entry k, 15 + k vertex 1
constexpr int kErrors = 29;
// the perturbation table: entry k < 14 is Sim3(+-delta e_d), d = k >> 1, +delta for even k; entry 14 is Sim3(0), which is what a
// vertex with _fix_scale gets along d = 6 (oplusImpl zeroes update[6] first, types_seven_dof_expmap.h:64-65)
constexpr int kTable = 15;

SE3_HD Sim3 table_entry(int k) {
    double add[7] = {0, 0, 0, 0, 0, 0, 0};
    const double delta = 1e-9;                                                 // base_binary_edge.hpp:147
    for (int d = 0; d < 7; d++)
        if (k < 14 && d == (k >> 1)) add[d] = (k & 1) ? -delta : delta;
    return sim3_exp(add);
}

// W.lu().solve(t) (sim3.h:217): Eigen's PartialPivLU of a 3x3 (the first largest |entry| of the column is the pivot, the column
// below it DIVIDED by the pivot, the trailing block updated), then the unit-lower and the upper substitution, column by column
SE3_HD void lu3_solve(double (*W)[3], const double* t, double* x) {
    int perm[3] = {0, 1, 2};
    for (int k = 0; k < 3; k++) {
        int p = k;
        double big = fabs(W[k][k]);
        for (int i = k + 1; i < 3; i++)
            if (fabs(W[i][k]) > big) { big = fabs(W[i][k]); p = i; }
        if (p != k) {
            for (int j = 0; j < 3; j++) { const double h = W[k][j]; W[k][j] = W[p][j]; W[p][j] = h; }
            const int h = perm[k]; perm[k] = perm[p]; perm[p] = h;
        }
        if (big != 0.0)
            for (int i = k + 1; i < 3; i++) W[i][k] /= W[k][k];
        for (int i = k + 1; i < 3; i++)
            for (int j = k + 1; j < 3; j++) W[i][j] -= W[i][k] * W[k][j];
    }
    double y[3] = {t[perm[0]], t[perm[1]], t[perm[2]]};
    y[1] -= W[1][0] * y[0];
    y[2] -= W[2][0] * y[0];
    y[2] -= W[2][1] * y[1];
    x[2] = y[2] / W[2][2];
    y[0] -= W[0][2] * x[2];
    y[1] -= W[1][2] * x[2];
    x[1] = y[1] / W[1][1];
    y[0] -= W[0][1] * x[1];
    x[0] = y[0] / W[0][0];
}

// Sim3::log (sim3.h:148-230) -> omega, upsilon, sigma
SE3_HD void sim3_log(const Sim3& S, double* res) {
    const double sigma = log(S.s);                                             // :151
    double R[3][3];                                                            // :160, Eigen's Quaternion::toRotationMatrix
    {
        const double tx = 2 * S.qx, ty = 2 * S.qy, tz = 2 * S.qz;
        const double twx = tx * S.qw, twy = ty * S.qw, twz = tz * S.qw, txx = tx * S.qx, txy = ty * S.qx, txz = tz * S.qx;
        const double tyy = ty * S.qy, tyz = tz * S.qy, tzz = tz * S.qz;
        R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
        R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
        R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
    }
    const double d = 0.5 * (((R[0][0] + R[1][1]) + R[2][2]) - 1);              // :161
    const double dR[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};   // deltaR (se3_ops.hpp:40-47)
    const double eps = 0.00001;
    const bool small_angle = d > 1 - eps;
    double f = 0.5, theta = 0;
    if (!small_angle) {                                                        // :181-183, :203-204
        theta = acos(d);
        f = theta / (2 * sqrt(1 - d * d));
    }
    const double ox = f * dR[0], oy = f * dR[1], oz = f * dR[2];
    double A, B, C;
    if (fabs(sigma) < eps) {                                                   // :169
        C = 1;
        if (small_angle) { A = 1. / 2.; B = 1. / 6.; }                         // :176-177
        else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / theta2;                                     // :185
            B = (theta - sin(theta)) / (theta2 * theta);                       // :186
        }
    } else {
        C = (S.s - 1) / sigma;                                                 // :191
        if (small_angle) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;                              // :198
            B = (((0.5 * sigma2 - sigma) + 1) * S.s) / (sigma2 * sigma);       // :199
        } else {
            const double theta2 = theta * theta;
            const double a = S.s * sin(theta), b = S.s * cos(theta);           // :207-208
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);                   // :210
            B = ((C - ((b - 1) * sigma + a * theta) / c) * 1.) / theta2;       // :211
        }
    }
    const double O[3][3] = {{0, -oz, oy}, {oz, 0, -ox}, {-oy, ox, 0}};         // skew (se3_ops.hpp:27-38)
    double W[3][3];                                                            // :215: A*Omega + (B*Omega)*Omega + C*I
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double p = ((B * O[i][0]) * O[0][j] + (B * O[i][1]) * O[1][j]) + (B * O[i][2]) * O[2][j];
            W[i][j] = (A * O[i][j] + p) + C * (i == j ? 1.0 : 0.0);
        }
    const double t[3] = {S.tx, S.ty, S.tz};
    lu3_solve(W, t, res + 3);                                                  // :217
    res[0] = ox; res[1] = oy; res[2] = oz;
    res[6] = sigma;
}

// EdgeSim3::computeError: (C * v0 * v1^-1).log()
SE3_HD void edge_error(const Sim3& C, const Sim3& v0, const Sim3& v1, double* e) {
    sim3_log(sim3_mul(sim3_mul(C, v0), sim3_inverse(v1)), e);
}

// chi2() = e . (Omega e) with the identity for Omega (base_edge.h:60)
SE3_HD double edge_chi2(const double* e) {
    double c = e[0] * e[0];
    for (int d = 1; d < 7; d++) c += e[d] * e[d];
    return c;
}

// Error vector `which` of an edge's linearisation (kErrors of them): push, oplus(+-delta e_d), computeError, pop
SE3_HD void edge_error_variant(const Sim3* tab, const Sim3& C, const Sim3& v0, const Sim3& v1, bool fix_scale0, bool fix_scale1,
                               int which, double* e) {
    if (which == 0) { edge_error(C, v0, v1, e); return; }
    const int side = which >= 15, k = which - (side ? 15 : 1);
    const bool fs = side ? fix_scale1 : fix_scale0;
    const Sim3 T = tab[(fs && (k >> 1) == 6) ? 14 : k];
    if (side) edge_error(C, v0, sim3_mul(T, v1), e);
    else edge_error(C, sim3_mul(T, v0), v1, e);
}

// _jacobianOplusX.col(col) = scalar * (error(+delta) - error(-delta)) (base_binary_edge.hpp:162-172), entry d; err: [kErrors][7]
SE3_HD double jacobian_entry(const double* err, int side, int d, int col) {
    const double scalar = 1.0 / (2 * 1e-9);                                    // :147-148
    const int plus = 1 + 14 * side + 2 * col;
    return scalar * (err[7 * plus + d] - err[7 * (plus + 1) + d]);
}

SE3_HD double dot7(const double* a, int sa, const double* b, int sb) {
    double t = a[0] * b[0];
    for (int d = 1; d < 7; d++) t += a[d * sa] * b[d * sb];
    return t;
}

// Plane q of constructQuadraticForm's terms; J: [2][7][7] as J[side][d][col], e: the base error.  A fixed end's planes are
// never asked for.
SE3_HD double quadratic_term(const double* J, const double* e, int q) {
    const double *A = J, *B = J + 49;
    if (q < kHab) {
        const double* M = q < kHbb ? A : B;
        int k = q < kHbb ? q : q - kHbb, a = 0;
        while (k >= 7 - a) { k -= 7 - a; a++; }
        return dot7(M + a, 7, M + a + k, 7);
    }
    if (q < kBa) return dot7(A + (q - kHab) / 7, 7, B + (q - kHab) % 7, 7);
    const double* M = q < kBb ? A : B;
    const int a = q < kBb ? q - kBa : q - kBb;
    double t = M[a] * -e[0];                                                   // omega_r = -omega * _error (:74)
    for (int d = 1; d < 7; d++) t += M[7 * d + a] * -e[d];
    return t;
}

// position of (r, c), r <= c, in a row-major upper triangle of a 7x7
SE3_HD int upper7(int r, int c) { return r * 7 - (r * (r - 1)) / 2 + (c - r); }

struct Outcome {
    int iterations, trials, rejected, solver_failures, stop;   // stop: 0 all iterations ran, 1 Terminate (:151-155), 2 _nBad (:164-167)
    double chi2_initial, chi2_final, lambda;
    double lambda_initial;   // what the first linearisation started from
};

// optimizer.optimize(max_it) (sparse_optimizer.cpp:376-389 with levenberg.cpp:61-170).  The backend keeps two copies of the state;
// push / pop is which copy is current.
//   be.linearise(cur, chi)                       computeActiveErrors + activeRobustChi2 + buildSystem at copy `cur`
//   be.trial(cur, lambda, chi, scale, solved)    setLambda, solve, update into copy cur ^ 1, the cost there, computeScale
// Both return 0 or an error code, which ends the loop and is returned.  lambda_init(be) is computeLambdaInit (:172-186), asked once,
// after the first linearisation.  stopped() is SparseOptimizer::terminate(), the caller's stop flag, asked where g2o asks it
// (sparse_optimizer.cpp:376, levenberg.cpp:149); o.stop = 3 when it ended the call.
template <typename Backend, typename LambdaInit, typename Stopped>
inline int levenberg(Backend& be, int max_it, bool any_edge, Outcome& o, LambdaInit lambda_init, Stopped stopped) {
    o = Outcome();
    int cur = 0, n_bad = 0;
    double lambda = 0, ni = 2;
    bool ok = any_edge;   // without an active edge there is nothing to optimise: zero iterations
    bool flag = false;
    for (int it = 0; it < max_it && !(flag = stopped()) && ok; it++) {
        double current = 0;
        if (int rc = be.linearise(cur, current)) return rc;
        double temp = current;
        const double ini = current;
        if (it == 0) {                                     // :93-97
            o.chi2_initial = current;
            lambda = o.lambda_initial = lambda_init(be);
            ni = 2;
            n_bad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            double scale = 0;
            int solved = 1;
            if (int rc = be.trial(cur, lambda, temp, scale, solved)) return rc;
            if (!solved) { temp = DBL_MAX; o.solver_failures++; }   // :126-127
            rho = current - temp;
            scale += 1e-3;                                 // :130-131
            rho /= scale;
            o.trials++;
            if (rho > 0 && std::isfinite(temp)) {               // :134-142
                const double y = 2 * rho - 1;
                double alpha = 1. - (y * y) * y;
                alpha = std::fmin(alpha, 2. / 3.);
                lambda *= std::fmax(1. / 3., alpha);
                ni = 2;
                current = temp;
                cur ^= 1;                                  // discardTop: the trial copy is the state
            } else {                                       // :143-147: pop = the trial copy is dropped
                lambda *= ni;
                ni *= 2;
                o.rejected++;
            }
            qmax++;
        } while (rho < 0 && qmax < 10 && !stopped());      // :149
        o.iterations++;
        o.chi2_final = current;
        if (qmax == 10 || rho == 0) { ok = false; o.stop = 1; continue; }   // :151-155
        if ((ini - current) * 1e3 < ini) n_bad++;          // :157-162
        else n_bad = 0;
        if (n_bad >= 3) { ok = false; o.stop = 2; }        // :164-167
    }
    if (flag && ok) o.stop = 3;
    if (o.iterations == 0) o.chi2_final = o.chi2_initial;
    o.lambda = lambda;
    be.current = cur;
    return 0;
}

// without a stop flag (OptimizeEssentialGraph sets none)
template <typename Backend, typename LambdaInit>
inline int levenberg(Backend& be, int max_it, bool any_edge, Outcome& o, LambdaInit lambda_init) {
    return levenberg(be, max_it, any_edge, o, lambda_init, [] { return false; });
}

// the 7-DoF form: computeLambdaInit returns the user value (:174-175), solver->setUserLambdaInit(1e-16) (Optimizer.cc:1423, :1698)
template <typename Backend>
inline int levenberg(Backend& be, int max_it, bool any_edge, Outcome& o) {
    return levenberg(be, max_it, any_edge, o, [](Backend&) { return 1e-16; });
}

}  // namespace eg
}  // namespace msorb
