// Optimizer::InertialOptimization (src/Optimizer.cc:3050-3227, :3230-3384, :3386-3491) after the gathering loops: the graph of
// EdgeInertialGS (src/G2oTypes.cc:596-718), EdgePriorAcc / EdgePriorGyro (include/G2oTypes.h:768-812, src/G2oTypes.cc:762-775) and the
// vertices VertexVelocity, VertexGyroBias, VertexAccBias, VertexGDir, VertexScale (include/G2oTypes.h:191-317), the quadratic form
// of a BaseMultiEdge (g2o/core/base_multi_edge.hpp:36-48, :171-222), Levenberg (optimization_algorithm_levenberg.cpp:61-195) and
// Gauss-Newton (optimization_algorithm_gauss_newton.cpp:50-93) under sparse_optimizer.cpp:354-419.  One statement of the arithmetic
// for the device (inertial_opt.hip) and the host (tests/inertial_opt_main.cc): plain arithmetic in the order the reference writes
// it, a product of small matrices the row-by-column sum left to right, nothing contracted (-ffp-contract=off).  DESIGN.md section 19.
//
// EdgeInertial, which tracking and LocalInertialBA use, is this edge with Rwg = I, s = 1 and free poses: bias_corrected, the SO3
// functions, edge_error and the quadratic form are what those routines start from.
//
// The preintegration's bias correction is FLOAT (src/ImuTypes.cc:277-308), one rounded operation per reference operator.  Both
// NormalizeRotation (ImuTypes.cc:34-37 in float, G2oTypes.h:68-71 in double) are U V^T of Eigen's JacobiSVD, whose bits are not
// pinned: fixed here as the one-sided Jacobi of essential_graph4_device.h, in float with FLT_EPSILON / FLT_MIN for the first.
//
// The routine is a template over an executor that says who walks which edges and rows and how sums are added:
//   ex.tid(), ex.stride()   this executor's first item and the step to its next one (host: 0, 1; device: threadIdx.x, 256)
//   ex.barrier()            everything written before it is visible to every executor after it
//   ex.sum(v, n)            v[0, n), n <= kSumMax, added over all executors; everyone returns with the same bits.  A barrier.
//   ex.max1(v)              the largest v of all executors
#pragma once
#include <cfloat>
#include <cmath>
#include <stdint.h>

#include "../../include/msorb.h"
#include "essential_graph4_device.h"   // exp_so3, log_so3, mul33, mul33_bt, mul3v, dot3, SE3_HD
#include "levenberg_device.h"

#if defined(__HIP_DEVICE_COMPILE__)
// the linearisation, the 3x3 eliminations and the border's factorisation inlined into one loop overflow the register file (as in
// sim3_opt_device.h): on the device they stay functions of their own
#define INERTIAL_OUT_OF_LINE __attribute__((noinline))
#else
#define INERTIAL_OUT_OF_LINE
#endif

namespace msorb {
namespace inertial {

using eg4::dot3;
using eg4::exp_so3;
using eg4::log_so3;
using eg4::mul33;
using eg4::mul3v;

// Columns of one edge's Jacobian in the order of its vertices (Optimizer.cc:3167-3174 without the two poses): VV1, VG, VA, VV2,
// VGDir, VS.  The upper triangle of the edge's 15x15 form is then what computeQuadraticForm writes (block (i, j) for i < j).
constexpr int kV1 = 0, kBg = 3, kBa = 6, kV2 = 9, kGd = 12, kSc = 14, kCols = 15;
constexpr int kEdgeB = 120, kEdgeW = 135;   // per edge: the upper triangle (row major), then b
constexpr int kBorderMax = 9, kRhs = kBorderMax + 1, kSumMax = 9;
constexpr int kMaxSweeps = 30;

SE3_HD int up15(int r, int c) { return r * kCols - (r * (r - 1)) / 2 + (c - r); }
SE3_HD double edge_h(const double* W, int a, int b) { return a <= b ? W[up15(a, b)] : W[up15(b, a)]; }

struct Globals { double Rwg[9], scale, bg[3], ba[3]; };

// which vertices are active and where the border's unknowns sit among the edge's columns (g2o orders the unknowns by vertex id:
// the velocities, then VG, VA, VGDir, VS)
struct Active { int fv, fb, fg, fs, m, bcol[kBorderMax]; };

struct Work {
    int n_kf, n_edges, n_rows;
    const msorb_inertial_keyframe* kf;
    const msorb_inertial_edge* edge;
    const int *row_kf, *e_prev, *e_next;   // inertial_plan.h
    double* v;                              // [2][3 n_kf]: the two copies of the velocities (push / pop)
    double* W;                              // [n_edges][kEdgeW]
    double* chi2;                           // [n_edges]
    double *D, *L, *U;                      // [n_rows][9]: the block-tridiagonal part, reduced in place
    double *R, *R0;                         // [n_rows][3][kRhs]: b and the border columns; R0 keeps what R held before the solve
    double* x;                              // [3 n_rows]: the solver's x, kept over a failed solve
};

// ---- float: Preintegrated::GetDeltaBias / GetDeltaRotation / GetDeltaVelocity / GetDeltaPosition (src/ImuTypes.cc:277-308)

SE3_HD float dot3f(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
SE3_HD void mul33f(const float* A, const float* B, float* C) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) C[3 * r + c] = dot3f(A[3 * r], A[3 * r + 1], A[3 * r + 2], B[c], B[3 + c], B[6 + c]);
}
SE3_HD void mul3vf(const float* A, const float* x, float* y) {
    for (int r = 0; r < 3; r++) y[r] = dot3f(A[3 * r], A[3 * r + 1], A[3 * r + 2], x[0], x[1], x[2]);
}

// NormalizeRotation (ImuTypes.cc:34-37): U V^T by eg4::normalize_rotation's one-sided Jacobi, in float
SE3_HD void normalize_rotation_f(const float* T, float* R) {
    float G[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int q = 0; q < 9; q++) G[q] = T[q];
    for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
        bool finished = true;
        for (int i = 0; i < 2; i++)
            for (int j = i + 1; j < 3; j++) {
                const float alpha = dot3f(G[i], G[3 + i], G[6 + i], G[i], G[3 + i], G[6 + i]);
                const float beta = dot3f(G[j], G[3 + j], G[6 + j], G[j], G[3 + j], G[6 + j]);
                const float gamma = dot3f(G[i], G[3 + i], G[6 + i], G[j], G[3 + j], G[6 + j]);
                const float thr = (2.0f * FLT_EPSILON) * sqrtf(alpha * beta);
                if (!(fabsf(gamma) > (thr > FLT_MIN ? thr : FLT_MIN))) continue;
                finished = false;
                const float tau = (beta - alpha) / (2.0f * gamma), w = sqrtf(tau * tau + 1.0f);
                const float t = tau >= 0.0f ? 1.0f / (tau + w) : 1.0f / (tau - w);
                const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
                for (int k = 0; k < 3; k++) {
                    const float gi = G[3 * k + i], gj = G[3 * k + j], vi = V[3 * k + i], vj = V[3 * k + j];
                    G[3 * k + i] = c * gi - s * gj;
                    G[3 * k + j] = s * gi + c * gj;
                    V[3 * k + i] = c * vi - s * vj;
                    V[3 * k + j] = s * vi + c * vj;
                }
            }
        if (finished) break;
    }
    for (int j = 0; j < 3; j++) {
        const float n = sqrtf(dot3f(G[j], G[3 + j], G[6 + j], G[j], G[3 + j], G[6 + j]));
        for (int k = 0; k < 3; k++) G[3 * k + j] /= n;
    }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[3 * r + c] = dot3f(G[3 * r], G[3 * r + 1], G[3 * r + 2], V[3 * c], V[3 * c + 1], V[3 * c + 2]);
}

// Sophus::SO3f::exp(w).matrix() (sophus/so3.hpp:583-619 through the quaternion, then Eigen's Quaternion::toRotationMatrix)
SE3_HD void so3f_exp_matrix(const float* w, float* R) {
    const float theta_sq = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    float imag, real;
    if (theta_sq < 1e-5f * 1e-5f) {                                            // Constants<float>::epsilon() squared
        const float theta_po4 = theta_sq * theta_sq;
        imag = (0.5f - (float)(1.0 / 48.0) * theta_sq) + (float)(1.0 / 3840.0) * theta_po4;
        real = (1.0f - (float)(1.0 / 8.0) * theta_sq) + (float)(1.0 / 384.0) * theta_po4;
    } else {
        const float theta = sqrtf(theta_sq), half_theta = 0.5f * theta;
        imag = sinf(half_theta) / theta;
        real = cosf(half_theta);
    }
    const float x = imag * w[0], y = imag * w[1], z = imag * w[2], qw = real;
    const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
    const float twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y,
                tzz = tz * z;
    R[0] = 1.0f - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0f - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0f - (txx + tyy);
}

// GetDeltaRotation / Velocity / Position(b) widened to double (G2oTypes.cc:631-633), and dbg of GetDeltaBias (:653-656).  The bias
// is IMU::Bias built from the double estimates narrowed to float (:628).
SE3_HD void bias_corrected(const msorb_inertial_edge& E, const Globals& G, double* dR, double* dV, double* dP, double* dbg) {
    float dbgf[3], dbaf[3], w[3], X[9], P[9], N[9], a[3], b[3];
    for (int k = 0; k < 3; k++) {
        dbaf[k] = (float)G.ba[k] - E.bias[k];
        dbgf[k] = (float)G.bg[k] - E.bias[3 + k];
        dbg[k] = (double)dbgf[k];
    }
    mul3vf(E.JRg, dbgf, w);
    so3f_exp_matrix(w, X);
    mul33f(E.dR, X, P);
    normalize_rotation_f(P, N);                                                // ImuTypes.cc:289
    for (int q = 0; q < 9; q++) dR[q] = (double)N[q];
    mul3vf(E.JVg, dbgf, a);
    mul3vf(E.JVa, dbaf, b);
    for (int k = 0; k < 3; k++) dV[k] = (double)((E.dV[k] + a[k]) + b[k]);     // :298
    mul3vf(E.JPg, dbgf, a);
    mul3vf(E.JPa, dbaf, b);
    for (int k = 0; k < 3; k++) dP[k] = (double)((E.dP[k] + a[k]) + b[k]);     // :307
}

// ---- double: the SO3 Jacobians of src/G2oTypes.cc (ExpSO3 and LogSO3 are essential_graph4_device.h's)

// RightJacobianSO3 (G2oTypes.cc:839-854): I - W (1 - cos d) / d2 + W W (d - sin d) / (d2 d)
SE3_HD void right_jacobian_so3(double x, double y, double z, double* J) {
    const double d2 = (x * x + y * y) + z * z, d = sqrt(d2);
    const double W[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
    if (d < 1e-5) { for (int q = 0; q < 9; q++) J[q] = q % 4 == 0 ? 1.0 : 0.0; return; }
    double WW[9];
    mul33(W, W, WW);
    const double a = 1.0 - cos(d), b = d - sin(d), c = d2 * d;
    for (int q = 0; q < 9; q++) J[q] = ((q % 4 == 0 ? 1.0 : 0.0) - (W[q] * a) / d2) + (WW[q] * b) / c;
}

// InverseRightJacobianSO3 (G2oTypes.cc:821-832): I + W / 2 + W W (1 / d2 - (1 + cos d) / (2 d sin d))
SE3_HD void inverse_right_jacobian_so3(double x, double y, double z, double* J) {
    const double d2 = (x * x + y * y) + z * z, d = sqrt(d2);
    const double W[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
    if (d < 1e-5) { for (int q = 0; q < 9; q++) J[q] = q % 4 == 0 ? 1.0 : 0.0; return; }
    double WW[9];
    mul33(W, W, WW);
    const double k = 1.0 / d2 - (1.0 + cos(d)) / ((2.0 * d) * sin(d));
    for (int q = 0; q < 9; q++) J[q] = ((q % 4 == 0 ? 1.0 : 0.0) + W[q] / 2) + WW[q] * k;
}

SE3_HD double gravity_value() { return (double)9.81f; }                       // const float GRAVITY_VALUE (ImuTypes.h:43)

// ---- EdgeInertialGS

// What computeError and linearizeOplus both form at one estimate
struct EdgeTerms { double Rbw1[9], eR[9], dbg[3], dv[3], dp[3], dt, s; };

// computeError (G2oTypes.cc:617-640).  v1, v2: the two velocities.  g, a member the reference sets here and reads in linearizeOplus
// (:676-678, for the pose's blocks only), is evaluated with the error at the same estimate.
SE3_HD void edge_error(const msorb_inertial_edge& E, const msorb_inertial_keyframe& k1, const msorb_inertial_keyframe& k2,
                       const double* v1, const double* v2, const Globals& G, double* e, EdgeTerms& T) {
    double dR[9], dV[3], dP[3], g[3], dRt[9], A[9], tv[3], tp[3], r[3];
    const double gI[3] = {0.0, 0.0, -gravity_value()};                         // :602
    bias_corrected(E, G, dR, dV, dP, T.dbg);
    mul3v(G.Rwg, gI, g);                                                       // :629
    const double s = G.scale, dt = (double)E.dT;                               // dt(pInt->dT) (:598)
    for (int r_ = 0; r_ < 3; r_++)
        for (int c = 0; c < 3; c++) { T.Rbw1[3 * r_ + c] = k1.Rwb[3 * c + r_]; dRt[3 * r_ + c] = dR[3 * c + r_]; }
    mul33(dRt, T.Rbw1, A);                                                     // :635
    mul33(A, k2.Rwb, T.eR);
    log_so3(T.eR, e);
    for (int k = 0; k < 3; k++) {
        T.dv[k] = v2[k] - v1[k];
        T.dp[k] = (k2.twb[k] - k1.twb[k]) - v1[k] * dt;
        tv[k] = s * T.dv[k] - g[k] * dt;                                       // :636
        tp[k] = s * T.dp[k] - ((g[k] * dt) * dt) / 2;                          // :637
    }
    mul3v(T.Rbw1, tv, r);
    for (int k = 0; k < 3; k++) e[3 + k] = r[k] - dV[k];
    mul3v(T.Rbw1, tp, r);
    for (int k = 0; k < 3; k++) e[6 + k] = r[k] - dP[k];
    T.dt = dt;
    T.s = s;
}

// chi2() = e . (Omega e) with the full information (base_edge.h:60); Oe = Omega e
SE3_HD double edge_chi2(const double* info, const double* e, double* Oe) {
    for (int r = 0; r < 9; r++) {
        double t = info[9 * r] * e[0];
        for (int c = 1; c < 9; c++) t += info[9 * r + c] * e[c];
        Oe[r] = t;
    }
    double chi = e[0] * Oe[0];
    for (int r = 1; r < 9; r++) chi += e[r] * Oe[r];
    return chi;
}

// linearizeOplus (G2oTypes.cc:642-718) for the vertices that can be free here: J [9][kCols].  The poses are fixed.
SE3_HD void edge_jacobian(const msorb_inertial_edge& E, const Globals& G, const double* e, const EdgeTerms& T, double* J) {
    for (int q = 0; q < 9 * kCols; q++) J[q] = 0.0;
    const double s = T.s, dt = T.dt, Gv = gravity_value();
    double invJr[9], nInv[9], eRt[9], A[9], B[9], RJ[9], JRg[9], w[3], r[3];
    inverse_right_jacobian_so3(e[0], e[1], e[2], invJr);                       // :670 (er = LogSO3(eR) is the error's)
    for (int q = 0; q < 9; q++) { nInv[q] = -invJr[q]; JRg[q] = (double)E.JRg[q]; }
    for (int r_ = 0; r_ < 3; r_++)
        for (int c = 0; c < 3; c++) eRt[3 * r_ + c] = T.eR[3 * c + r_];
    mul3v(JRg, T.dbg, w);
    right_jacobian_so3(w[0], w[1], w[2], RJ);
    mul33(nInv, eRt, A);                                                       // :689: ((-invJr eR^T) RJ) JRg
    mul33(A, RJ, B);
    mul33(B, JRg, A);
    double dG[6];                                                              // dGdTheta = Rwg Gm (:662-666), [3][2]
    for (int r_ = 0; r_ < 3; r_++) {
        dG[2 * r_] = (G.Rwg[3 * r_] * 0.0 + G.Rwg[3 * r_ + 1] * Gv) + G.Rwg[3 * r_ + 2] * 0.0;
        dG[2 * r_ + 1] = (G.Rwg[3 * r_] * -Gv + G.Rwg[3 * r_ + 1] * 0.0) + G.Rwg[3 * r_ + 2] * 0.0;
    }
    for (int r_ = 0; r_ < 3; r_++) {
        for (int c = 0; c < 3; c++) {
            const double Rb = T.Rbw1[3 * r_ + c];
            J[(3 + r_) * kCols + kV1 + c] = -s * Rb;                           // :684
            J[(6 + r_) * kCols + kV1 + c] = (-s * Rb) * dt;                    // :685
            J[r_ * kCols + kBg + c] = A[3 * r_ + c];
            J[(3 + r_) * kCols + kBg + c] = -(double)E.JVg[3 * r_ + c];        // :690
            J[(6 + r_) * kCols + kBg + c] = -(double)E.JPg[3 * r_ + c];        // :691
            J[(3 + r_) * kCols + kBa + c] = -(double)E.JVa[3 * r_ + c];        // :695
            J[(6 + r_) * kCols + kBa + c] = -(double)E.JPa[3 * r_ + c];        // :696
            J[(3 + r_) * kCols + kV2 + c] = s * Rb;                            // :707
        }
        for (int c = 0; c < 2; c++) {
            const double m1 = dot3(-T.Rbw1[3 * r_], -T.Rbw1[3 * r_ + 1], -T.Rbw1[3 * r_ + 2], dG[c], dG[2 + c], dG[4 + c]);
            const double m2 = dot3(-0.5 * T.Rbw1[3 * r_], -0.5 * T.Rbw1[3 * r_ + 1], -0.5 * T.Rbw1[3 * r_ + 2], dG[c], dG[2 + c], dG[4 + c]);
            J[(3 + r_) * kCols + kGd + c] = m1 * dt;                           // :711
            J[(6 + r_) * kCols + kGd + c] = (m2 * dt) * dt;                    // :712
        }
    }
    mul3v(T.Rbw1, T.dv, r);                                                    // :716
    for (int k = 0; k < 3; k++) J[(3 + k) * kCols + kSc] = r[k];
    mul3v(T.Rbw1, T.dp, r);                                                    // :717
    for (int k = 0; k < 3; k++) J[(6 + k) * kCols + kSc] = r[k];
}

// One inertial edge of one buildSystem: computeError, chi2, the robust kernel, linearizeOplus, constructQuadraticForm
// (base_multi_edge.hpp:36-48) and computeQuadraticForm (:171-222): AtO = A^T omega, the diagonal block AtO A, b += A^T omega_r, the
// blocks AtO B for the later vertices.  W: the edge's kEdgeW terms.  Returns rho[0]; chi2 = the edge's chi2().
INERTIAL_OUT_OF_LINE SE3_HD double edge_linearize(const msorb_inertial_edge& E, const msorb_inertial_keyframe& k1,
                                                  const msorb_inertial_keyframe& k2, const double* v1, const double* v2,
                                                  const Globals& G, bool robust, double& chi2, double* W) {
    double e[9], Oe[9], J[9 * kCols], rho0, rho1;
    EdgeTerms T;
    edge_error(E, k1, k2, v1, v2, G, e, T);
    chi2 = edge_chi2(E.info, e, Oe);
    se3::huber(chi2, 1.0, robust, rho0, rho1);                                 // rk->setDelta(1.f) (Optimizer.cc:3475)
    edge_jacobian(E, G, e, T, J);
    double wr[9];
    for (int k = 0; k < 9; k++) wr[k] = robust ? (-Oe[k]) * rho1 : -Oe[k];     // omega_r = -information * error; *= rho[1]
    for (int a = 0; a < kCols; a++) {
        double AtO[9];
        for (int c = 0; c < 9; c++) {
            double t = 0;
            for (int k = 0; k < 9; k++) {
                const double o = robust ? rho1 * E.info[9 * k + c] : E.info[9 * k + c];   // robustInformation (base_edge.h:96-100)
                const double p = J[k * kCols + a] * o;
                t = k == 0 ? p : t + p;
            }
            AtO[c] = t;
        }
        for (int b = a; b < kCols; b++) {
            double t = AtO[0] * J[b];
            for (int c = 1; c < 9; c++) t += AtO[c] * J[c * kCols + b];
            W[up15(a, b)] = t;
        }
        double t = J[a] * wr[0];
        for (int k = 1; k < 9; k++) t += J[k * kCols + a] * wr[k];
        W[kEdgeB + a] = t;
    }
    return rho0;
}

// computeError and chi2 alone (computeActiveErrors): returns rho[0]
SE3_HD double edge_cost(const msorb_inertial_edge& E, const msorb_inertial_keyframe& k1, const msorb_inertial_keyframe& k2,
                        const double* v1, const double* v2, const Globals& G, bool robust, double& chi2) {
    double e[9], Oe[9], rho0, rho1;
    EdgeTerms T;
    edge_error(E, k1, k2, v1, v2, G, e, T);
    chi2 = edge_chi2(E.info, e, Oe);
    se3::huber(chi2, 1.0, robust, rho0, rho1);
    return rho0;
}

// The two prior edges are active only while their bias vertex is free: initializeOptimization takes an edge with
// !allVerticesFixed() (sparse_optimizer.cpp:234-237), and a unary edge's only vertex is the bias, which bFixedVel fixes
// (Optimizer.cc:3096-3106).  A prior on a fixed bias enters neither the cost nor the count of active edges.
SE3_HD bool priors_active(const msorb_inertial_problem& P) { return P.with_priors != 0 && P.free_biases != 0; }

// EdgePriorAcc / EdgePriorGyro (G2oTypes.h:778-781, :802-805): error = bprior - estimate with bprior = 0, information p I;
// chi2 = e . (Omega e)
SE3_HD double prior_chi2(const double* bias, double p) {
    double chi = 0;
    for (int k = 0; k < 3; k++) {
        const double e = 0.0 - bias[k];
        chi = k == 0 ? e * (p * e) : chi + e * (p * e);
    }
    return chi;
}

// the vertex updates: VertexGyroBias / VertexAccBias += u (G2oTypes.h:227-231, :248-252), GDirection::Update (:264-267),
// VertexScale (:314-316).  xb: the border's part of x, in the order of A.bcol.
SE3_HD void update_globals(const Globals& in, const Active& A, const double* xb, Globals& out) {
    out = in;
    int k = 0;
    if (A.fb) {
        for (int c = 0; c < 3; c++) out.bg[c] = in.bg[c] + xb[k + c];
        for (int c = 0; c < 3; c++) out.ba[c] = in.ba[c] + xb[k + 3 + c];
        k += 6;
    }
    if (A.fg) {
        double Ex[9];
        exp_so3(xb[k], xb[k + 1], 0.0, Ex);
        mul33(in.Rwg, Ex, out.Rwg);
        k += 2;
    }
    if (A.fs) out.scale = in.scale * exp(xb[k]);
}

// ---- the linear system

// Unpivoted square-root-free L D L^T of the n x n matrix whose upper triangle is in A (row major, stride ld), n <= kBorderMax:
// Lf[i][j] (j < i) the factor, rinv[j] = 1 / D_j.  false: a pivot that is not > 0 ("solver failed").
SE3_HD bool ldlt_factor(int n, const double* A, int ld, double* Lf, double* rinv) {
    for (int j = 0; j < n; j++) {
        double v[kBorderMax];
        double d = A[j * ld + j];
        for (int m = 0; m < j; m++) { v[m] = Lf[j * kBorderMax + m] * Lf[m * kBorderMax + m]; d -= Lf[j * kBorderMax + m] * v[m]; }
        if (!(d > 0)) return false;
        Lf[j * kBorderMax + j] = d;
        rinv[j] = 1.0 / d;
        for (int i = j + 1; i < n; i++) {
            double s = A[j * ld + i];
            for (int m = 0; m < j; m++) s -= Lf[i * kBorderMax + m] * v[m];
            Lf[i * kBorderMax + j] = s * rinv[j];
        }
    }
    return true;
}
// x = (L D L^T)^-1 b; b and x with stride sb / sx, may be the same
SE3_HD void ldlt_apply(int n, const double* Lf, const double* rinv, const double* b, int sb, double* x, int sx) {
    double y[kBorderMax];
    for (int i = 0; i < n; i++) {
        double s = b[i * sb];
        for (int m = 0; m < i; m++) s -= Lf[i * kBorderMax + m] * y[m];
        y[i] = s;
    }
    for (int i = n - 1; i >= 0; i--) {
        double s = y[i] * rinv[i];
        for (int m = i + 1; m < n; m++) s -= Lf[m * kBorderMax + i] * x[m * sx];
        x[i * sx] = s;
    }
}

// One side of a cyclic-reduction step for kept row i and its eliminated neighbour j: Y = D_j^-1 [L_j | U_j | R_j], then
// Dn -= C Y_far, near coupling = -(C Y_near), Rn -= C Y_R, where C couples i to j (L_i for j below i, U_i for j above).
// lower: j = i - s.  false: D_j has a pivot that is not > 0.
INERTIAL_OUT_OF_LINE SE3_HD bool reduce_side(const Work& K, int nr, int i, int j, bool lower, double* Dn, double* Cn, double* Rn) {
    double Lf[kBorderMax * kBorderMax], rinv[3];
    if (!ldlt_factor(3, K.D + 9 * j, 3, Lf, rinv)) return false;
    const double* C = (lower ? K.L : K.U) + 9 * i;
    const double *Lj = K.L + 9 * j, *Uj = K.U + 9 * j, *Rj = K.R + 3 * kRhs * j;
    for (int c = 0; c < 6 + nr; c++) {
        // column c of [L_j | U_j | R_j]
        const double* src = c < 3 ? Lj + c : c < 6 ? Uj + (c - 3) : Rj + (c - 6);
        const int st = c < 6 ? 3 : kRhs;
        double y[3], cy[3];
        ldlt_apply(3, Lf, rinv, src, st, y, 1);
        mul3v(C, y, cy);
        // towards i: the block of row j that couples back to i (U_j below, L_j above) lands on D_i; the other one is the new coupling
        const bool back = lower ? (c >= 3 && c < 6) : c < 3;
        for (int r = 0; r < 3; r++) {
            if (c >= 6) Rn[r * kRhs + (c - 6)] -= cy[r];
            else if (back) Dn[3 * r + (c % 3)] -= cy[r];
            else Cn[3 * r + (c % 3)] = -cy[r];
        }
    }
    return true;
}

// (T + lambda I) X = R for the block-tridiagonal T in K.D / K.L / K.U, nr right-hand sides, by block cyclic reduction: at stride s
// the rows i = 0 mod 2s eliminate their neighbours i - s and i + s, one executor per kept row; then row 0 alone, then the
// eliminated rows stride by stride downwards.  X replaces R.  Returns this executor's "met a bad pivot"; the caller adds them.
template <typename Exec>
SE3_HD double cyclic_reduction(Exec& ex, const Work& K, int nr) {
    const int n = K.n_rows;
    double bad = 0;
    int s = 1;
    for (; s < n; s *= 2) {
        for (int i = ex.tid() * 2 * s; i < n; i += ex.stride() * 2 * s) {
            double Dn[9], Ln[9], Un[9], Rn[3 * kRhs];
            for (int q = 0; q < 9; q++) { Dn[q] = K.D[9 * i + q]; Ln[q] = 0; Un[q] = 0; }
            for (int q = 0; q < 3 * kRhs; q++) Rn[q] = K.R[3 * kRhs * i + q];
            if (i - s >= 0 && !reduce_side(K, nr, i, i - s, true, Dn, Ln, Rn)) bad = 1;
            if (i + s < n && !reduce_side(K, nr, i, i + s, false, Dn, Un, Rn)) bad = 1;
            for (int q = 0; q < 9; q++) { K.D[9 * i + q] = Dn[q]; K.L[9 * i + q] = Ln[q]; K.U[9 * i + q] = Un[q]; }
            for (int q = 0; q < 3 * kRhs; q++) K.R[3 * kRhs * i + q] = Rn[q];
        }
        ex.barrier();
    }
    for (; s >= 1; s /= 2) {                                                   // s >= n: row 0; below: the rows i = s mod 2s
        for (int i = s >= n ? ex.tid() * 2 * s : s + ex.tid() * 2 * s; i < n; i += ex.stride() * 2 * s) {
            double Lf[kBorderMax * kBorderMax], rinv[3];
            if (!ldlt_factor(3, K.D + 9 * i, 3, Lf, rinv)) { bad = 1; continue; }
            double* Ri = K.R + 3 * kRhs * i;
            for (int c = 0; c < nr; c++) {
                double rhs[3] = {Ri[c], Ri[kRhs + c], Ri[2 * kRhs + c]};
                if (s < n) {
                    const double* Xl = K.R + 3 * kRhs * (i - s);
                    const double xl[3] = {Xl[c], Xl[kRhs + c], Xl[2 * kRhs + c]};
                    double t[3];
                    mul3v(K.L + 9 * i, xl, t);
                    for (int r = 0; r < 3; r++) rhs[r] -= t[r];
                    if (i + s < n) {
                        const double* Xu = K.R + 3 * kRhs * (i + s);
                        const double xu[3] = {Xu[c], Xu[kRhs + c], Xu[2 * kRhs + c]};
                        mul3v(K.U + 9 * i, xu, t);
                        for (int r = 0; r < 3; r++) rhs[r] -= t[r];
                    }
                }
                ldlt_apply(3, Lf, rinv, rhs, 1, Ri + c, kRhs);
            }
        }
        ex.barrier();
    }
    return bad;
}

// v[0, n) = the sum over items [0, count) of term(item, q), every executor walking its items in ascending order, in chunks of
// kSumMax through ex.sum
template <typename Exec, typename F>
SE3_HD void tree_sum(Exec& ex, int count, int n, double* out, F term) {
    for (int q0 = 0; q0 < n; q0 += kSumMax) {
        const int nq = n - q0 < kSumMax ? n - q0 : kSumMax;
        double acc[kSumMax];
        for (int j = 0; j < kSumMax; j++) acc[j] = 0;
        for (int it = ex.tid(); it < count; it += ex.stride())
            for (int j = 0; j < nq; j++) acc[j] += term(it, q0 + j);
        ex.sum(acc, nq);
        for (int j = 0; j < nq; j++) out[q0 + j] = acc[j];
    }
}

// position q of the border's sums: the upper triangle of the m x m block (row major), then its m entries of b
SE3_HD void border_index(int m, int q, int& a, int& b) {
    a = 0;
    if (q >= (m * (m + 1)) / 2) { a = q - (m * (m + 1)) / 2; b = -1; return; }
    while (q >= m - a) { q -= m - a; a++; }
    b = a + q;
}

struct Solved { bool ok; double scale; };

// One state of the optimisation: what every executor holds with equal bits
struct State {
    Globals G[2];          // the two copies (push / pop); cur says which is the estimate
    int cur;
    double C[(kBorderMax * (kBorderMax + 1)) / 2 + kBorderMax];   // the border's block and b, as the last linearisation left them
    double xb[kBorderMax];                                        // the border's part of x
};

// computeActiveErrors + activeRobustChi2 at copy `which`: the priors first (g2o's edge list: epa, epg, then the inertial edges)
template <typename Exec>
SE3_HD double active_chi2(Exec& ex, const Work& K, const msorb_inertial_problem& P, const State& S, int which, bool robust) {
    const Globals& G = S.G[which];
    const double* v = K.v + (size_t)which * 3 * K.n_kf;
    double c[1] = {0};
    for (int e = ex.tid(); e < K.n_edges; e += ex.stride()) {
        const msorb_inertial_edge& E = K.edge[e];
        c[0] += edge_cost(E, K.kf[E.kf_prev], K.kf[E.kf_cur], v + 3 * E.kf_prev, v + 3 * E.kf_cur, G, robust, K.chi2[e]);
    }
    ex.sum(c, 1);
    double chi = 0;
    if (priors_active(P)) chi = prior_chi2(G.ba, P.prior_a) + prior_chi2(G.bg, P.prior_g);
    return chi + c[0];
}

// computeActiveErrors + buildSystem at the current copy: every edge's terms into K.W, the border's sums into S.C.  Returns
// activeRobustChi2; max_diag = the largest |H(j, j)| (computeLambdaInit, levenberg.cpp:172-186).
template <typename Exec>
SE3_HD double linearise(Exec& ex, const Work& K, const msorb_inertial_problem& P, const Active& A, State& S, bool robust, double& max_diag) {
    const Globals& G = S.G[S.cur];
    const double* v = K.v + (size_t)S.cur * 3 * K.n_kf;
    double c[1] = {0};
    for (int e = ex.tid(); e < K.n_edges; e += ex.stride()) {
        const msorb_inertial_edge& E = K.edge[e];
        c[0] += edge_linearize(E, K.kf[E.kf_prev], K.kf[E.kf_cur], v + 3 * E.kf_prev, v + 3 * E.kf_cur, G, robust, K.chi2[e],
                               K.W + (size_t)kEdgeW * e);
    }
    ex.sum(c, 1);                                                              // (its barrier publishes K.W)
    const int m = A.m, nq = (m * (m + 1)) / 2 + m;
    tree_sum(ex, K.n_edges, nq, S.C, [&](int e, int q) {
        int a, b;
        border_index(m, q, a, b);
        const double* W = K.W + (size_t)kEdgeW * e;
        return b < 0 ? W[kEdgeB + A.bcol[a]] : edge_h(W, A.bcol[a], A.bcol[b]);
    });
    double chi = 0;
    if (priors_active(P)) {
        chi = prior_chi2(G.ba, P.prior_a) + prior_chi2(G.bg, P.prior_g);
        if (A.fb) {                                                            // linearizeOplus = I (G2oTypes.cc:762-775); b += -(Omega e)
            const int tri = (m * (m + 1)) / 2;
            for (int k = 0; k < 3; k++) {
                int q = 0;
                for (int a = 0; a < k; a++) q += m - a;
                S.C[q] += P.prior_g;                                           // VG: rows 0..2 of the border
                S.C[tri + k] += -(P.prior_g * (0.0 - G.bg[k]));
                q = 0;
                for (int a = 0; a < 3 + k; a++) q += m - a;
                S.C[q] += P.prior_a;                                           // VA: rows 3..5
                S.C[tri + 3 + k] += -(P.prior_a * (0.0 - G.ba[k]));
            }
        }
    }
    double md = 0;
    if (A.fv)
        for (int r = ex.tid(); r < K.n_rows; r += ex.stride())
            for (int k = 0; k < 3; k++) {
                double d = 0;
                if (K.e_prev[r] >= 0) d = K.W[(size_t)kEdgeW * K.e_prev[r] + up15(kV2 + k, kV2 + k)];
                if (K.e_next[r] >= 0) d += K.W[(size_t)kEdgeW * K.e_next[r] + up15(kV1 + k, kV1 + k)];
                md = fmax(fabs(d), md);
            }
    md = ex.max1(md);
    for (int a = 0, q = 0; a < m; q += m - a, a++) md = fmax(fabs(S.C[q]), md);
    max_diag = md;
    return chi + c[0];
}

// setLambda, solve: x into K.x and S.xb when every pivot was positive (they keep what they held otherwise), and computeScale's
// sum of x_j (lambda x_j + b_j) (levenberg.cpp:188-195)
template <typename Exec>
SE3_HD Solved solve(Exec& ex, const Work& K, const Active& A, State& S, double lambda) {
    const int m = A.m, nr = m + 1, n = A.fv ? K.n_rows : 0;
    // each velocity's at most two contributions, the previous edge first
    for (int r = ex.tid(); r < n; r += ex.stride()) {
        const double* Wp = K.e_prev[r] >= 0 ? K.W + (size_t)kEdgeW * K.e_prev[r] : nullptr;
        const double* Wn = K.e_next[r] >= 0 ? K.W + (size_t)kEdgeW * K.e_next[r] : nullptr;
        double* R0 = K.R0 + 3 * kRhs * r;
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) {
                double d = 0;
                if (Wp) d = edge_h(Wp, kV2 + a, kV2 + b);
                if (Wn) d = Wp ? d + edge_h(Wn, kV1 + a, kV1 + b) : edge_h(Wn, kV1 + a, kV1 + b);
                K.D[9 * r + 3 * a + b] = a == b ? d + lambda : d;
                K.U[9 * r + 3 * a + b] = Wn ? Wn[up15(kV1 + a, kV2 + b)] : 0.0;
                K.L[9 * r + 3 * a + b] = Wp ? Wp[up15(kV1 + b, kV2 + a)] : 0.0;
            }
            for (int c = 0; c < nr; c++) {
                double t = 0;
                if (c == 0) {
                    if (Wp) t = Wp[kEdgeB + kV2 + a];
                    if (Wn) t = Wp ? t + Wn[kEdgeB + kV1 + a] : Wn[kEdgeB + kV1 + a];
                } else {
                    const int col = A.bcol[c - 1];
                    if (Wp) t = edge_h(Wp, kV2 + a, col);
                    if (Wn) t = Wp ? t + edge_h(Wn, kV1 + a, col) : edge_h(Wn, kV1 + a, col);
                }
                R0[a * kRhs + c] = t;
                K.R[3 * kRhs * r + a * kRhs + c] = t;
            }
        }
    }
    ex.barrier();
    double bad[1] = {0};
    if (n > 0) bad[0] = cyclic_reduction(ex, K, nr);
    ex.sum(bad, 1);
    bool ok = !(bad[0] > 0);
    // the border: C + lambda I - B^T T^-1 B and b_c - B^T T^-1 b, the rows added in a fixed order
    const int tri = (m * (m + 1)) / 2, nq = tri + m;
    double Sc[(kBorderMax * (kBorderMax + 1)) / 2 + kBorderMax];
    tree_sum(ex, n, nq, Sc, [&](int r, int q) {
        int a, b;
        border_index(m, q, a, b);
        const double *B = K.R0 + 3 * kRhs * r, *X = K.R + 3 * kRhs * r;
        const int cb = b < 0 ? 0 : 1 + b;
        return dot3(B[1 + a], B[kRhs + 1 + a], B[2 * kRhs + 1 + a], X[cb], X[kRhs + cb], X[2 * kRhs + cb]);
    });
    double y[kBorderMax];
    for (int k = 0; k < kBorderMax; k++) y[k] = 0;
    if (ok && m > 0) {
        double M[kBorderMax * kBorderMax], rhs[kBorderMax], Lf[kBorderMax * kBorderMax], rinv[kBorderMax];
        for (int a = 0, q = 0; a < m; a++)
            for (int b = a; b < m; b++, q++) M[a * kBorderMax + b] = (a == b ? S.C[q] + lambda : S.C[q]) - Sc[q];
        for (int a = 0; a < m; a++) rhs[a] = S.C[tri + a] - Sc[tri + a];
        ok = ldlt_factor(m, M, kBorderMax, Lf, rinv);
        if (ok) ldlt_apply(m, Lf, rinv, rhs, 1, y, 1);
    }
    if (ok) {
        for (int k = 0; k < m; k++) S.xb[k] = y[k];
        for (int r = ex.tid(); r < n; r += ex.stride()) {
            const double* X = K.R + 3 * kRhs * r;
            for (int a = 0; a < 3; a++) {
                double t = X[a * kRhs];
                for (int k = 0; k < m; k++) t -= X[a * kRhs + 1 + k] * y[k];
                K.x[3 * r + a] = t;
            }
        }
    }
    ex.barrier();
    double sc[1] = {0};
    for (int r = ex.tid(); r < n; r += ex.stride())
        for (int a = 0; a < 3; a++) sc[0] += K.x[3 * r + a] * (lambda * K.x[3 * r + a] + K.R0[3 * kRhs * r + a * kRhs]);
    ex.sum(sc, 1);
    for (int k = 0; k < m; k++) sc[0] += S.xb[k] * (lambda * S.xb[k] + S.C[tri + k]);
    return Solved{ok, sc[0]};
}

// update(x) from copy `from` into copy `to` (oplus of every active vertex)
template <typename Exec>
SE3_HD void update(Exec& ex, const Work& K, const Active& A, State& S, int from, int to) {
    const double* vi = K.v + (size_t)from * 3 * K.n_kf;
    double* vo = K.v + (size_t)to * 3 * K.n_kf;
    if (A.fv)
        for (int r = ex.tid(); r < K.n_rows; r += ex.stride())
            for (int a = 0; a < 3; a++) vo[3 * K.row_kf[r] + a] = vi[3 * K.row_kf[r] + a] + K.x[3 * r + a];
    Globals G;
    update_globals(S.G[from], A, S.xb, G);
    S.G[to] = G;
    ex.barrier();
}

// optimizer.optimize(its) of either algorithm and what the callers read afterwards: the velocities in K.v's first copy.  Every executor returns with the whole result; whoever leads writes it.
template <typename Exec>
SE3_HD void optimize(Exec& ex, const Work& K, const msorb_inertial_problem& P, msorb_inertial_result& out) {
    Active A;
    const bool any = K.n_edges > 0;
    A.fv = (P.free_velocities && any) ? 1 : 0;
    A.fb = (P.free_biases && (any || P.with_priors)) ? 1 : 0;                  // (a free bias under a prior is active without inertial edges)
    A.fg = (P.free_gdir && any) ? 1 : 0;
    A.fs = (P.free_scale && any) ? 1 : 0;
    A.m = 0;
    for (int k = 0; k < kBorderMax; k++) A.bcol[k] = 0;
    if (A.fb) for (int k = 0; k < 6; k++) A.bcol[A.m++] = kBg + k;
    if (A.fg) for (int k = 0; k < 2; k++) A.bcol[A.m++] = kGd + k;
    if (A.fs) A.bcol[A.m++] = kSc;
    State S;
    for (int q = 0; q < 9; q++) S.G[0].Rwg[q] = P.Rwg[q];
    S.G[0].scale = P.scale;
    for (int k = 0; k < 3; k++) { S.G[0].bg[k] = P.bg[k]; S.G[0].ba[k] = P.ba[k]; }
    S.G[1] = S.G[0];
    S.cur = 0;
    for (int k = 0; k < kBorderMax; k++) S.xb[k] = 0;
    for (int r = ex.tid(); r < 3 * K.n_rows; r += ex.stride()) K.x[r] = 0;     // the solver's x starts at zero
    for (int k = ex.tid(); k < K.n_kf; k += ex.stride())                       // VertexVelocity(pKF): both copies
        for (int a = 0; a < 3; a++) K.v[3 * k + a] = K.v[(size_t)3 * K.n_kf + 3 * k + a] = K.kf[k].v[a];
    ex.barrier();
    const bool robust = P.huber != 0;
    int status = 0, iterations = 0, rejected = 0;
    double chi2_initial = 0;
    if (!(A.fv || A.m > 0)) {
        status = 1;                                                            // sparse_optimizer.cpp:356-359: returns -1
    } else if (P.algorithm == 1) {                                             // gauss_newton.cpp:50-93 under sparse_optimizer.cpp:376
        bool ok = true;
        for (int i = 0; i < P.iterations && ok; i++) {
            double md;
            const double chi = linearise(ex, K, P, A, S, robust, md);
            if (i == 0) chi2_initial = chi;
            const Solved sv = solve(ex, K, A, S, 0.0);
            update(ex, K, A, S, S.cur, S.cur ^ 1);                             // :85: also when the solve failed
            S.cur ^= 1;
            iterations++;
            if (!sv.ok) { ok = false; status = 2; }                            // :89-92 Fail
        }
    } else {                                                                   // levenberg_device.h: levenberg.cpp:61-170
        const lm::Counts n = lm::levenberg(
            P.iterations, P.user_lambda_init != 0, 1e3,                        // setUserLambdaInit(1e3) (Optimizer.cc:3069, :3245)
            [&](double& max_diagonal) { return linearise(ex, K, P, A, S, robust, max_diagonal); },
            [&](double lambda, bool& solved, double& scale) {
                const Solved sv = solve(ex, K, A, S, lambda);                  // :103-110
                update(ex, K, A, S, S.cur, S.cur ^ 1);                         // :115
                solved = sv.ok;
                scale = sv.scale;
                return active_chi2(ex, K, P, S, S.cur ^ 1, robust);            // :123-124
            },
            [&]() { S.cur ^= 1; });
        iterations = n.iterations;
        rejected = n.rejected;
        chi2_initial = n.chi2_initial;
    }
    const double chi2_final = active_chi2(ex, K, P, S, S.cur, robust);         // leaves every edge's chi2 at the returned estimate
    if (iterations == 0) chi2_initial = chi2_final;
    if (S.cur == 1) {                                                          // the caller reads copy 0
        for (int r = ex.tid(); r < 3 * K.n_kf; r += ex.stride()) K.v[r] = K.v[(size_t)3 * K.n_kf + r];
        ex.barrier();
    }
    if (ex.tid() == 0) {
        const Globals& G = S.G[S.cur];
        for (int q = 0; q < 9; q++) out.Rwg[q] = G.Rwg[q];
        out.scale = G.scale;
        for (int k = 0; k < 3; k++) { out.bg[k] = G.bg[k]; out.ba[k] = G.ba[k]; }
        out.chi2_initial = chi2_initial;
        out.chi2_final = chi2_final;
        out.status = status;
        out.iterations = iterations;
        out.rejected_trials = rejected;
        out.n_active_edges = K.n_edges + (priors_active(P) ? 2 : 0);
    }
}

// ---- host only: the information matrix of EdgeInertialGS's constructor (G2oTypes.cc:604-612)
//
//   Info = C.block<9,9>(0,0).cast<double>().inverse(); Info = (Info + Info^T) / 2; SelfAdjointEigenSolver; eigenvalues below 1e-12
//   to 0; Info = V diag(eigs) V^T
//
// in plain double: Gauss-Jordan elimination with partial pivoting for the inverse, a cyclic Jacobi eigen-decomposition, the
// recomposition as the product (V diag) V^T, row by column left to right.  Parity with Eigen's PartialPivLU inverse and its
// tridiagonal QL solver is NOT pinned; tests/inertial_opt_cases.py's `info` variant measures what another pair of solvers moves.
// C: the 9x9 block as floats, row major with stride ldc (15 for Preintegrated::C).  info: 81 doubles, not exactly symmetric.
// false: a pivot of the inverse is zero or not finite (Eigen would return non-finite entries).
#if !defined(__HIP_DEVICE_COMPILE__)
inline bool info_from_covariance(const float* C, int ldc, double* info) {
    double M[9][18];
    for (int r = 0; r < 9; r++)
        for (int c = 0; c < 9; c++) { M[r][c] = (double)C[r * ldc + c]; M[r][9 + c] = r == c ? 1.0 : 0.0; }
    for (int c = 0; c < 9; c++) {
        int p = c;
        for (int r = c + 1; r < 9; r++)
            if (fabs(M[r][c]) > fabs(M[p][c])) p = r;
        if (!(fabs(M[p][c]) > 0) || !std::isfinite(M[p][c])) return false;
        for (int k = 0; k < 18; k++) { const double t = M[c][k]; M[c][k] = M[p][k]; M[p][k] = t; }
        const double d = M[c][c];
        for (int k = 0; k < 18; k++) M[c][k] = M[c][k] / d;
        for (int r = 0; r < 9; r++) {
            if (r == c) continue;
            const double f = M[r][c];
            for (int k = 0; k < 18; k++) M[r][k] = M[r][k] - f * M[c][k];
        }
    }
    double A[9][9], V[9][9];
    for (int r = 0; r < 9; r++)
        for (int c = 0; c < 9; c++) { A[r][c] = (M[r][9 + c] + M[c][9 + r]) / 2; V[r][c] = r == c ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0, diag = 0;
        for (int r = 0; r < 9; r++) {
            diag += A[r][r] * A[r][r];
            for (int c = r + 1; c < 9; c++) off += A[r][c] * A[r][c];
        }
        if (!(sqrt(off) > 1e-17 * sqrt(diag))) break;
        for (int p = 0; p < 8; p++)
            for (int q = p + 1; q < 9; q++) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 9; k++) {                                  // A <- A G
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 9; k++) {                                  // A <- G^T A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 9; k++) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    for (int r = 0; r < 9; r++)
        for (int c = 0; c < 9; c++) {
            double t = 0;
            for (int k = 0; k < 9; k++) {
                const double eig = A[k][k] < 1e-12 ? 0.0 : A[k][k];            // :608-610
                const double term = (V[r][k] * eig) * V[c][k];
                t = k == 0 ? term : t + term;
            }
            info[9 * r + c] = t;
        }
    return true;
}
#endif

}  // namespace inertial
}  // namespace msorb
