// Optimizer::OptimizeSim3 (src/Optimizer.cc:1986-2242 and :2244-2429) after the gathering loops: g2o's Sim3 (types/sim3.h),
// VertexSim3Expmap::oplusImpl (OptimizableTypes.h:158-167), the two edges (:183-190, :204-211), the NUMERIC Jacobian this fork
// gets from BaseBinaryEdge::linearizeOplus (core/base_binary_edge.hpp:131-205; OptimizableTypes.h:192,213 comment the analytic
// one out), the 7x7 system, the Levenberg loop (core/optimization_algorithm_levenberg.cpp:61-195 under sparse_optimizer.cpp:376)
// and the two classifications.  One statement of the arithmetic for the device (sim3_opt_kernel, sim3_opt.hip) and the host
// (tests/sim3_opt_main.cc): plain double arithmetic in the order written, nothing contracted (-ffp-contract=off).
//
// The routine is a template over an executor that says how the pairs are walked, how the sums are added and who computes the
// perturbed estimates; everything else is the same text for both.  DESIGN.md section 13.
//
// mTc of both edges is the identity (EdgeSim3ProjectXYZ(Sophus::SE3d Tc = Sophus::SE3d()), and OptimizeSim3 passes nothing):
// a unit quaternion (0, 0, 0, 1) and a zero translation change no bit of the mapped point, so it is left out.
#pragma once
#include <stdint.h>
#if !defined(__HIPCC__)
#include <float.h>
#endif

#include "../../include/msorb.h"
#include "se3_device.h"

// The perturbed transforms are the same for every edge, so a compiler that sees the whole map hoists all 28 of them (224 doubles)
// out of it and spills.  A compiler-only fence (no instruction, no effect on the arithmetic) keeps each read where it is used.
#if defined(__HIP_DEVICE_COMPILE__)
#define SIM3_OPT_KEEP_LOADS_HERE() asm volatile("" ::: "memory")
// The fully unrolled 7x7 factorisation and Sim3(update) inlined into the trial loop, next to the sums and the resident pairs, are
// what overflows the register file: on the device they stay functions of their own.
#define SIM3_OPT_OUT_OF_LINE __attribute__((noinline))
#else
#define SIM3_OPT_KEEP_LOADS_HERE()
#define SIM3_OPT_OUT_OF_LINE
#endif

namespace msorb {
namespace sim3opt {

using se3::Pose;

struct Sim3 { double qx, qy, qz, qw, tx, ty, tz, s; };   // g2o::Sim3: r, t, s.  Nothing normalises r (sim3.h:59-62, :266-272)

// one correspondence as the reference holds it before the widening: P3D1c / P3D2c (:2058,:2066), obs1 / obs2, invSigmaSquare1 / 2
struct Pair { float P1[3], P2[3], o1[2], o2[2], w1, w2; };

struct Cam { double fx, fy, cx, cy; };   // Pinhole's mvParameters[0..3], floats widened (Pinhole.cpp:35-41)

constexpr int kSums = 36;         // 28 (upper triangle of H, row major) + 7 (b) + 1 (the cost)
constexpr int kPerturbed = 14;    // +delta and -delta along each of the 7 directions

// Sim3(const Vector7d& update) (sim3.h:70-142): the four (sigma, theta) branches, Quaterniond(R), W = A Omega + B Omega^2 + C I
SIM3_OPT_OUT_OF_LINE SE3_HD Sim3 sim3_exp(const double* u) {
    const double ox = u[0], oy = u[1], oz = u[2], sigma = u[6];
    const double theta = sqrt((ox * ox + oy * oy) + oz * oz);                  // :82
    const double O[3][3] = {{0, -oz, oy}, {oz, 0, -ox}, {-oy, ox, 0}};         // :83 skew
    const double s = exp(sigma);                                               // :84
    double O2[3][3], R[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) O2[i][j] = (O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j];   // :85
    const double eps = 0.00001;
    const bool small_theta = theta < eps;
    double sn = 0, cs = 1;
    if (!small_theta) sincos(theta, &sn, &cs);
    double A, B, C;
    if (fabs(sigma) < eps) {                                                   // :92
        C = 1;
        if (small_theta) { A = 1. / 2.; B = 1. / 6.; }                         // :97-98
        else {
            const double theta2 = theta * theta;
            A = (1 - cs) / theta2;                                             // :104
            B = (theta - sn) / (theta2 * theta);                               // :105
        }
    } else {
        C = (s - 1) / sigma;                                                   // :111
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;                                // :115
            B = (((0.5 * sigma2 - sigma) + 1) * s) / (sigma2 * sigma);         // :116
        } else {
            const double a = s * sn, b = s * cs;                               // :125-126
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);                   // :131
            B = ((C - ((b - 1) * sigma + a * theta) / c) * 1.) / theta2;       // :132
        }
    }
    if (small_theta) {                                                         // :99, :117
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
    } else {                                                                   // :106, :121
        const double a = sn / theta, b = (1 - cs) / (theta * theta);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + a * O[i][j]) + b * O2[i][j];
    }
    double q[4];
    se3::quaternion_of_matrix(R, q);                                           // :136
    double W[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) W[i][j] = (A * O[i][j] + B * O2[i][j]) + C * (i == j ? 1.0 : 0.0);   // :140
    Sim3 E;
    E.qx = q[0]; E.qy = q[1]; E.qz = q[2]; E.qw = q[3];
    E.tx = (W[0][0] * u[3] + W[0][1] * u[4]) + W[0][2] * u[5];                 // :141
    E.ty = (W[1][0] * u[3] + W[1][1] * u[4]) + W[1][2] * u[5];
    E.tz = (W[2][0] * u[3] + W[2][1] * u[4]) + W[2][2] * u[5];
    E.s = s;
    return E;
}

SE3_HD Pose rotation_of(const Sim3& S) { return Pose{S.qx, S.qy, S.qz, S.qw, 0, 0, 0}; }

// Sim3::map (sim3.h:144-146): s*(r*xyz) + t
SE3_HD void sim3_map(const Sim3& S, double X, double Y, double Z, double& x, double& y, double& z) {
    se3::rotate(rotation_of(S), X, Y, Z, x, y, z);
    x = S.s * x + S.tx; y = S.s * y + S.ty; z = S.s * z + S.tz;
}

// Sim3::operator* (sim3.h:266-272); Eigen's quaternion product
SE3_HD Sim3 sim3_mul(const Sim3& a, const Sim3& b) {
    Sim3 r;
    r.qw = ((a.qw * b.qw - a.qx * b.qx) - a.qy * b.qy) - a.qz * b.qz;
    r.qx = ((a.qw * b.qx + a.qx * b.qw) + a.qy * b.qz) - a.qz * b.qy;
    r.qy = ((a.qw * b.qy + a.qy * b.qw) + a.qz * b.qx) - a.qx * b.qz;
    r.qz = ((a.qw * b.qz + a.qz * b.qw) + a.qx * b.qy) - a.qy * b.qx;
    double x, y, z;
    se3::rotate(rotation_of(a), b.tx, b.ty, b.tz, x, y, z);
    r.tx = a.s * x + a.tx; r.ty = a.s * y + a.ty; r.tz = a.s * z + a.tz;
    r.s = a.s * b.s;
    return r;
}

// Sim3::inverse (sim3.h:233-236): Sim3(r.conjugate(), r.conjugate()*((-1./s)*t), 1./s)
SE3_HD Sim3 sim3_inverse(const Sim3& S) {
    Sim3 r;
    r.qx = -S.qx; r.qy = -S.qy; r.qz = -S.qz; r.qw = S.qw;
    const double f = -1. / S.s;
    se3::rotate(rotation_of(r), f * S.tx, f * S.ty, f * S.tz, r.tx, r.ty, r.tz);
    r.s = 1. / S.s;
    return r;
}

// VertexSim3Expmap::oplusImpl (OptimizableTypes.h:158-167).  update[6] = 0 is written INTO the caller's vector, which is the
// solver's x: computeScale (levenberg.cpp:188-195) reads the zero afterwards.
SE3_HD Sim3 sim3_oplus(const Sim3& S, double* update, bool fix_scale) {
    if (fix_scale) update[6] = 0;
    return sim3_mul(sim3_exp(update), S);
}

// The 14 estimates of one linearisation and their inverses (base_binary_edge.hpp:157-170: push, oplus(+-delta e_d), pop):
// entry k (0..13) is direction k >> 1, +delta for even k and -delta for odd k.
SE3_HD void sim3_perturbed(const Sim3& S, bool fix_scale, int k, Sim3& plus, Sim3& plus_inverse) {
    double add[7] = {0, 0, 0, 0, 0, 0, 0};
    const double delta = 1e-9;                                                 // :147
    for (int d = 0; d < 7; d++)
        if (d == (k >> 1)) add[d] = (k & 1) ? -delta : delta;
    plus = sim3_oplus(S, add, fix_scale);
    plus_inverse = sim3_inverse(plus);                                         // e21: estimate().inverse() at every evaluation
}

// computeError of either edge for one transform: obs - project(T.map(X)) (OptimizableTypes.h:183-190 with T = the estimate and
// X = P3D2c, :204-211 with T = its inverse and X = P3D1c); Pinhole::project(Vector3d) (Pinhole.cpp:35-41)
SE3_HD void edge_error(const Sim3& T, const Cam& c, const float* X, const float* obs, double* e) {
    double x, y, z;
    sim3_map(T, (double)X[0], (double)X[1], (double)X[2], x, y, z);
    e[0] = (double)obs[0] - ((c.fx * x) / z + c.cx);
    e[1] = (double)obs[1] - ((c.fy * y) / z + c.cy);
}

// chi2() = e . (Omega e), Omega = I * invSigma2 (base_edge.h:60)
SE3_HD double edge_chi2(const double* e, double w) { return e[0] * (w * e[0]) + e[1] * (w * e[1]); }

// One edge of one solve(): computeError, chi2, the robust kernel, linearizeOplus by central differences, constructQuadraticForm
// (base_binary_edge.hpp:47-120; the Sim3 vertex is vertex 1, `to`, its Jacobian B).  tab: the 14 transforms this edge type maps
// with (the perturbed estimates for e12, their inverses for e21).  Adds the edge's 36 terms to S.
SE3_HD void edge_linearize(const Sim3& T, const Sim3* tab, const Cam& c, const float* X, const float* obs, float wf, double delta,
                           bool robust, double& chi2, double* S) {
    const double w = (double)wf;
    double e[2], J[2][7], rho0, rho1;
    edge_error(T, c, X, obs, e);
    chi2 = edge_chi2(e, w);
    se3::huber(chi2, delta, robust, rho0, rho1);
    S[35] += rho0;                                                             // activeRobustChi2 (levenberg.cpp:82)
    const double scalar = 1.0 / (2 * 1e-9);                                    // :147-148
SE3_UNROLL
    for (int d = 0; d < 7; d++) {
        double ep[2], em[2];
        SIM3_OPT_KEEP_LOADS_HERE();
        edge_error(tab[2 * d], c, X, obs, ep);                                 // errorBak = _error
        edge_error(tab[2 * d + 1], c, X, obs, em);                             // errorBak -= _error
        J[0][d] = scalar * (ep[0] - em[0]);                                    // :172
        J[1][d] = scalar * (ep[1] - em[1]);
    }
    const double wr = rho1 * w;                                                // robustInformation (base_edge.h:96-100)
    const double r0 = (-(w * e[0])) * rho1, r1 = (-(w * e[1])) * rho1;         // omega_r = -omega * _error; omega_r *= rho[1]
    int k = 0;
SE3_UNROLL
    for (int a = 0; a < 7; a++) {
SE3_UNROLL
        for (int b = a; b < 7; b++, k++) S[k] += (J[0][a] * wr) * J[0][b] + (J[1][a] * wr) * J[1][b];   // B^T weightedOmega B
        S[28 + a] += J[0][a] * r0 + J[1][a] * r1;                              // B^T omega_r
    }
}

// Square-root-free Cholesky (L D L^T, no pivoting) of H + lambda I (the upper triangle in Hu, row major), then the substitutions:
// solve6 of pose_opt.hip for 7 unknowns.  false = a pivot that is not positive; x keeps what it held.
SIM3_OPT_OUT_OF_LINE SE3_HD bool solve7(const double* Hu, double lambda, const double* b, double* x) {
    double L[7][7], r[7];
    int k = 0;
    for (int i = 0; i < 7; i++)
        for (int j = i; j < 7; j++) { L[j][i] = Hu[k++]; if (i == j) L[i][i] += lambda; }
    for (int j = 0; j < 7; j++) {
        double v[7];
        double d = L[j][j];
        for (int m = 0; m < j; m++) { v[m] = L[j][m] * L[m][m]; d -= L[j][m] * v[m]; }
        if (!(d > 0)) return false;
        L[j][j] = d;
        r[j] = 1.0 / d;
        for (int i = j + 1; i < 7; i++) {
            double s = L[i][j];
            for (int m = 0; m < j; m++) s -= L[i][m] * v[m];
            L[i][j] = s * r[j];
        }
    }
    double y[7];
    for (int i = 0; i < 7; i++) {
        double s = b[i];
        for (int m = 0; m < i; m++) s -= L[i][m] * y[m];
        y[i] = s;
    }
    for (int i = 6; i >= 0; i--) {
        double s = y[i] * r[i];
        for (int m = i + 1; m < 7; m++) s -= L[m][i] * x[m];
        x[i] = s;
    }
    return true;
}

// optimizer.optimize(max_it) over the pairs whose flag is 0 (sparse_optimizer.cpp:354-419 with levenberg.cpp:61-170: pose_opt.hip's
// loop widened to 7).  Every pass leaves the edges' chi2 in the per-pair state: the classification after the first run reads the
// error of the LAST TRIAL, also when that trial was popped (the stale-error rule of DESIGN.md section 9).
//
// Exec:  for_each_pair(f)   f(const Pair&, double* chi2 /* [2]: e12, e21 */, uint8_t& flag) over the executor's share of the pairs,
//                           ascending
//        sum<N>(v)          v[0, N) added over all executors; everyone returns with the same bits
//        perturbed(S, fix)  -> the table of sim3_perturbed: [0, 14) the estimates, [14, 28) their inverses
template <typename Exec>
SE3_HD void levenberg(Exec& ex, Sim3& S, const Cam& c1, const Cam& c2, double delta, bool robust, bool fix_scale, int max_it,
                      int& n_solve, int& n_rejected) {
    double lambda = 0, ni = 2;
    int n_bad_steps = 0;
    bool ok = true;
    double x[7] = {0, 0, 0, 0, 0, 0, 0};
    n_solve = n_rejected = 0;
    for (int i = 0; i < max_it && ok; i++) {                                   // sparse_optimizer.cpp:376
        double Sm[kSums];
SE3_UNROLL
        for (int k = 0; k < kSums; k++) Sm[k] = 0;
        const Sim3* tab = ex.perturbed(S, fix_scale);
        const Sim3 Sinv = sim3_inverse(S);
        ex.for_each_pair([&](const Pair& p, double* chi2, uint8_t& flag) {     // g2o's edge list: e12 of a pair, then its e21
            if (flag) return;
            edge_linearize(S, tab, c1, p.P2, p.o1, p.w1, delta, robust, chi2[0], Sm);
            edge_linearize(Sinv, tab + kPerturbed, c2, p.P1, p.o2, p.w2, delta, robust, chi2[1], Sm);
        });
        ex.template sum<kSums>(Sm);
        double current = Sm[35], temp = current;
        const double ini = current;
        double Hu[28], b[7];                                                   // the solver's copy: the sums themselves stay in registers
SE3_UNROLL
        for (int k = 0; k < 28; k++) Hu[k] = Sm[k];
SE3_UNROLL
        for (int k = 0; k < 7; k++) b[k] = Sm[28 + k];
        if (i == 0) {                                                          // computeLambdaInit (:172-186), _tau = 1e-5
            double max_diag = 0;
            for (int j = 0, k = 0; j < 7; k += 7 - j, j++) max_diag = fmax(fabs(Hu[k]), max_diag);
            lambda = 1e-5 * max_diag;
            ni = 2;
            n_bad_steps = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            const Sim3 backup = S;                                             // push (:103)
            const bool ok2 = solve7(Hu, lambda, b, x);                         // :109-110
            S = sim3_oplus(S, x, fix_scale);                                   // :115 (zeroes x[6] under fix_scale)
            const Sim3 Ti = sim3_inverse(S);
            double c[1] = {0};
            ex.for_each_pair([&](const Pair& p, double* chi2, uint8_t& flag) {
                if (flag) return;
                double e[2], rho0, rho1;
                edge_error(S, c1, p.P2, p.o1, e);                              // :123
                chi2[0] = edge_chi2(e, (double)p.w1);
                se3::huber(chi2[0], delta, robust, rho0, rho1);
                c[0] += rho0;                                                  // :124
                edge_error(Ti, c2, p.P1, p.o2, e);
                chi2[1] = edge_chi2(e, (double)p.w2);
                se3::huber(chi2[1], delta, robust, rho0, rho1);
                c[0] += rho0;
            });
            ex.template sum<1>(c);
            temp = c[0];
            if (!ok2) temp = DBL_MAX;                                          // :126-127
            rho = current - temp;
            double scale = 0;                                                  // computeScale (:188-195)
            for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + b[j]);
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && isfinite(temp)) {                                   // :134-142
                const double y = 2 * rho - 1;
                double alpha = 1. - (y * y) * y;                               // pow(2 rho - 1, 3)
                alpha = fmin(alpha, 2. / 3.);
                const double factor = fmax(1. / 3., alpha);
                lambda *= factor;
                ni = 2;
                current = temp;
            } else {                                                           // :143-147
                lambda *= ni;
                ni *= 2;
                S = backup;
                n_rejected++;
            }
            qmax++;
        } while (rho < 0 && qmax < 10);                                        // :149
        n_solve++;
        if (qmax == 10 || rho == 0) { ok = false; continue; }                  // :151-155 Terminate
        if ((ini - current) * 1e3 < ini) n_bad_steps++;                        // :157-162: this fork's _nBad stop
        else n_bad_steps = 0;
        if (n_bad_steps >= 3) ok = false;                                      // :164-167
    }
}

// Optimizer.cc:2172-2241 / :2363-2428.  Flags: 0 kept, 1 bad at the first classification, 2 bad at the final one.  Every executor
// returns with the whole result; whoever leads writes it.
template <typename Exec>
SE3_HD void optimize_sim3(Exec& ex, const msorb_sim3_opt_problem& P, msorb_sim3_opt_result& R) {
    const int n = P.n;
    const Cam c1{(double)P.cam1[0], (double)P.cam1[1], (double)P.cam1[2], (double)P.cam1[3]};
    const Cam c2{(double)P.cam2[0], (double)P.cam2[1], (double)P.cam2[2], (double)P.cam2[3]};
    const double th2 = (double)P.th2;                                          // `chi2() > th2`: the float widened
    const double delta = (double)(float)sqrt((double)P.th2);                   // const float deltaHuber = sqrt(th2) (:2029, :2291)
    const bool fix_scale = P.fix_scale != 0;
    const Sim3 S0{P.q[0], P.q[1], P.q[2], P.q[3], P.t[0], P.t[1], P.t[2], P.s};
    Sim3 S = S0;
    int iterations[2] = {-1, -1}, rejected[2] = {-1, -1};
    int n_bad = 0, n_in = 0, status = 1;
    if (n >= 1) {                                                              // optimize(5) (:2174, :2365), also below the minimum
        levenberg(ex, S, c1, c2, delta, true, fix_scale, P.its[0], iterations[0], rejected[0]);
        double bad[1] = {0};
        ex.for_each_pair([&](const Pair&, double* chi2, uint8_t& flag) {       // :2179-2203: chi2() as the last pass left it
            flag = (chi2[0] > th2 || chi2[1] > th2) ? 1 : 0;
            bad[0] += flag;
        });
        ex.template sum<1>(bad);
        n_bad = (int)bad[0];
    }
    if (!(n - n_bad < P.min_pairs)) {                                          // :2211-2212, :2397-2398: return 0 before g2oS12 is written
        status = 0;
        if (n - n_bad > 0)                                                     // a fresh run without the kernel: lambda starts again
            levenberg(ex, S, c1, c2, delta, false, fix_scale, n_bad > 0 ? P.its[1] : P.its[2], iterations[1], rejected[1]);
        else
            iterations[1] = rejected[1] = 0;
        const Sim3 Sinv = sim3_inverse(S);
        double in[1] = {0};
        ex.for_each_pair([&](const Pair& p, double* chi2, uint8_t& flag) {     // :2220-2235: computeError, then chi2()
            if (flag) return;
            double e[2];
            edge_error(S, c1, p.P2, p.o1, e);
            chi2[0] = edge_chi2(e, (double)p.w1);
            edge_error(Sinv, c2, p.P1, p.o2, e);
            chi2[1] = edge_chi2(e, (double)p.w2);
            if (chi2[0] > th2 || chi2[1] > th2) flag = 2;
            else in[0] += 1;
        });
        ex.template sum<1>(in);
        n_in = (int)in[0];
    } else {
        S = S0;
    }
    if (ex.leader()) {
        R.q[0] = S.qx; R.q[1] = S.qy; R.q[2] = S.qz; R.q[3] = S.qw;
        R.t[0] = S.tx; R.t[1] = S.ty; R.t[2] = S.tz;
        R.s = S.s;
        R.status = status;
        R.n_pairs = n;
        R.n_bad = n_bad;
        R.n_in = n_in;
        for (int k = 0; k < 2; k++) { R.iterations[k] = iterations[k]; R.rejected_trials[k] = rejected[k]; }
    }
}

}  // namespace sim3opt
}  // namespace msorb
