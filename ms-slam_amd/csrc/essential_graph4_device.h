// Optimizer::OptimizeEssentialGraph4DoF (src/Optimizer.cc:5174-5458) after the gathering loops: the 4-DoF pose graph of
// VertexPose4DoF / Edge4DoF (include/G2oTypes.h:74-110, 155-189, 817-843; src/G2oTypes.cc:25-71, 121-146, 222-256, 777-814) with the
// NUMERIC Jacobian of BaseBinaryEdge::linearizeOplus (core/base_binary_edge.hpp:131-203), constructQuadraticForm's terms with the
// information diag(1e3, 1e3, 1, 1, 1, 1) and no kernel (:55-90), and the Levenberg loop of essential_graph_device.h started from
// computeLambdaInit (optimization_algorithm_levenberg.cpp:172-186).  One statement of the arithmetic for the device
// (essential_graph4.hip) and the host (tests/essential_graph4_main.cc): plain double arithmetic in the order written, a product of
// small matrices the row-by-column sum left to right, nothing contracted (-ffp-contract=off).  DESIGN.md section 18.
//
// NormalizeRotation (G2oTypes.h:68-71) is U V^T of Eigen's JacobiSVD, whose bits are not pinned.  Fixed here: one-sided Jacobi on
// the columns g_0, g_1, g_2 of the matrix, the pairs (0,1) (0,2) (1,2) in that order, a pair rotated when
// |g_i . g_j| > max(DBL_MIN, 2 eps sqrt(|g_i|^2 |g_j|^2)), sweeps until one passes without a rotation or kMaxSweeps are done;
// U = the columns divided by their norms, V the accumulated rotations.
#pragma once
#include <cfloat>
#include <cmath>

#include "essential_graph_device.h"   // eg::levenberg, eg::Outcome, SE3_HD

namespace msorb {
namespace eg4 {

// one vertex's estimate (an ImuCamPose as far as Edge4DoF and UpdateW use it), kState doubles
constexpr int kDR = 0, kTwb = 9, kRcw = 12, kTcw = 21, kIts = 24, kState = 26;
// the error vectors of one linearisation: 0 the base error, 1 + k vertex 0 perturbed, 9 + k vertex 1; k = 2 column + (1: -delta)
constexpr int kErrors = 17;
// the rotations of the perturbations: ExpSO3(0, 0, +delta), ExpSO3(0, 0, -delta), ExpSO3(0, 0, 0)
constexpr int kTable = 3;
// planes of the edge-major linearisation: A^T O A and B^T O B (upper triangles, row major), A^T O B (full), A^T (-O e), B^T (-O e)
constexpr int kHaa = 0, kHbb = 10, kHab = 20, kBa = 36, kBb = 40, kPlanes = 44;
constexpr int kMaxSweeps = 30;

// matLambda (Optimizer.cc:5240-5243): (0, 0) is set twice and (2, 2) never
SE3_HD double information(int d) { return d < 2 ? 1e3 : 1.0; }

SE3_HD double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
// C = A B, C = A B^T, y = A x (row major)
SE3_HD void mul33(const double* A, const double* B, double* C) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) C[3 * r + c] = dot3(A[3 * r], A[3 * r + 1], A[3 * r + 2], B[c], B[3 + c], B[6 + c]);
}
SE3_HD void mul33_bt(const double* A, const double* B, double* C) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) C[3 * r + c] = dot3(A[3 * r], A[3 * r + 1], A[3 * r + 2], B[3 * c], B[3 * c + 1], B[3 * c + 2]);
}
SE3_HD void mul3v(const double* A, const double* x, double* y) {
    for (int r = 0; r < 3; r++) y[r] = dot3(A[3 * r], A[3 * r + 1], A[3 * r + 2], x[0], x[1], x[2]);
}

// NormalizeRotation: U V^T of T = U S V^T by the one-sided Jacobi described above
SE3_HD void normalize_rotation(const double* T, double* R) {
    double G[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int q = 0; q < 9; q++) G[q] = T[q];
    for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
        bool finished = true;
        for (int i = 0; i < 2; i++)
            for (int j = i + 1; j < 3; j++) {
                const double alpha = dot3(G[i], G[3 + i], G[6 + i], G[i], G[3 + i], G[6 + i]);
                const double beta = dot3(G[j], G[3 + j], G[6 + j], G[j], G[3 + j], G[6 + j]);
                const double gamma = dot3(G[i], G[3 + i], G[6 + i], G[j], G[3 + j], G[6 + j]);
                const double thr = (2.0 * DBL_EPSILON) * sqrt(alpha * beta);
                if (!(fabs(gamma) > (thr > DBL_MIN ? thr : DBL_MIN))) continue;
                finished = false;
                const double tau = (beta - alpha) / (2.0 * gamma), w = sqrt(tau * tau + 1.0);
                const double t = tau >= 0.0 ? 1.0 / (tau + w) : 1.0 / (tau - w);
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; k++) {
                    const double gi = G[3 * k + i], gj = G[3 * k + j], vi = V[3 * k + i], vj = V[3 * k + j];
                    G[3 * k + i] = c * gi - s * gj;
                    G[3 * k + j] = s * gi + c * gj;
                    V[3 * k + i] = c * vi - s * vj;
                    V[3 * k + j] = s * vi + c * vj;
                }
            }
        if (finished) break;
    }
    for (int j = 0; j < 3; j++) {
        const double n = sqrt(dot3(G[j], G[3 + j], G[6 + j], G[j], G[3 + j], G[6 + j]));
        for (int k = 0; k < 3; k++) G[3 * k + j] /= n;
    }
    mul33_bt(G, V, R);
}

// ExpSO3 (G2oTypes.cc:782-798)
SE3_HD void exp_so3(double x, double y, double z, double* R) {
    const double d2 = (x * x + y * y) + z * z, d = sqrt(d2);
    const double W[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
    double res[9];
    if (d < 1e-5) {                                                            // :790: I + W + (0.5 W) W
        double hW[9], WW[9];
        for (int q = 0; q < 9; q++) hW[q] = 0.5 * W[q];
        mul33(hW, W, WW);
        for (int q = 0; q < 9; q++) res[q] = ((q % 4 == 0 ? 1.0 : 0.0) + W[q]) + WW[q];
    } else {                                                                   // :795: I + (W sin d) / d + ((W W)(1 - cos d)) / d2
        double WW[9];
        mul33(W, W, WW);
        const double sn = sin(d), cm = 1.0 - cos(d);
        for (int q = 0; q < 9; q++) res[q] = ((q % 4 == 0 ? 1.0 : 0.0) + (W[q] * sn) / d) + (WW[q] * cm) / d2;
    }
    normalize_rotation(res, R);
}

// LogSO3 (G2oTypes.cc:800-814) with its three exits
SE3_HD void log_so3(const double* R, double* w) {
    const double tr = (R[0] + R[4]) + R[8];
    w[0] = (R[7] - R[5]) / 2; w[1] = (R[2] - R[6]) / 2; w[2] = (R[3] - R[1]) / 2;
    const double costheta = (tr - 1.0) * 0.5;
    if (costheta > 1 || costheta < -1) return;
    const double theta = acos(costheta), s = sin(theta);
    if (fabs(s) < 1e-5) return;
    for (int k = 0; k < 3; k++) w[k] = (theta * w[k]) / s;
}

// the estimate either constructor leaves (G2oTypes.cc:25-71, :121-146): DR = I, its = 0, Rcw / tcw as handed in
SE3_HD void state_init(const double* Rcw, const double* tcw, const double* twb, double* st) {
    for (int q = 0; q < 9; q++) { st[kDR + q] = q % 4 == 0 ? 1.0 : 0.0; st[kRcw + q] = Rcw[q]; }
    for (int k = 0; k < 3; k++) { st[kTwb + k] = twb[k]; st[kTcw + k] = tcw[k]; }
    st[kIts] = 0.0;
    st[kIts + 1] = 0.0;
}

// UpdateW's camera pose (G2oTypes.cc:231, :248-255): Rwb = DR Rwb0, Rbw = Rwb^T, tbw = -Rbw twb, Rcw = Rcb Rbw, tcw = Rcb tbw + tcb
SE3_HD void camera_pose(const double* DR, const double* twb, const double* Rwb0, const double* Rcb, const double* tcb, double* Rcw,
                        double* tcw) {
    double Rwb[9], Rbw[9], tbw[3];
    mul33(DR, Rwb0, Rwb);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Rbw[3 * r + c] = Rwb[3 * c + r];
    mul3v(Rbw, twb, tbw);
    for (int k = 0; k < 3; k++) tbw[k] = -tbw[k];
    mul33(Rcb, Rbw, Rcw);
    mul3v(Rcb, tbw, tcw);
    for (int k = 0; k < 3; k++) tcw[k] = tcw[k] + tcb[k];
}

// VertexPose4DoF::oplusImpl -> ImuCamPose::UpdateW({0, 0, u0, u1, u2, u3}) (G2oTypes.h:178-188, G2oTypes.cc:222-256); dR is
// ExpSO3(0, 0, u0), handed in so that the perturbations take theirs from the table.  `in` and `out` may not overlap.
SE3_HD void update_w(const double* in, const double* dR, const double* ut, const double* Rwb0, const double* Rcb, const double* tcb,
                     double* out) {
    mul33(dR, in + kDR, out + kDR);                                            // :230
    for (int k = 0; k < 3; k++) out[kTwb + k] = in[kTwb + k] + ut[k];          // :233
    camera_pose(out + kDR, out + kTwb, Rwb0, Rcb, tcb, out + kRcw, out + kTcw);
    double its = in[kIts] + 1.0;                                               // :236-245, after Rwb was formed: only later updates
    if (its >= 5.0) {                                                          // see it (NormalizeRotation(DR) discards its result)
        out[kDR + 2] = 0.0; out[kDR + 5] = 0.0; out[kDR + 6] = 0.0; out[kDR + 7] = 0.0;
        its = 0.0;
    }
    out[kIts] = its;
    out[kIts + 1] = 0.0;
}

// Edge4DoF::computeError (G2oTypes.h:831-836); meas: dRij[9], dtij[3]
SE3_HD void edge_error(const double* Rcw_i, const double* tcw_i, const double* Rcw_j, const double* tcw_j, const double* meas, double* e) {
    double Rij[9], Re[9], twj[3], t[3];
    mul33_bt(Rcw_i, Rcw_j, Rij);
    mul33_bt(Rij, meas, Re);
    log_so3(Re, e);
    for (int r = 0; r < 3; r++) twj[r] = -dot3(Rcw_j[r], Rcw_j[3 + r], Rcw_j[6 + r], tcw_j[0], tcw_j[1], tcw_j[2]);
    mul3v(Rcw_i, twj, t);
    for (int k = 0; k < 3; k++) e[3 + k] = (t[k] + tcw_i[k]) - meas[9 + k];
}

// chi2() = e . (Omega e)
SE3_HD double edge_chi2(const double* e) {
    double c = e[0] * (information(0) * e[0]);
    for (int d = 1; d < 6; d++) c += e[d] * (information(d) * e[d]);
    return c;
}

// the camera pose of a vertex after push, oplus(+-delta e_col), k = 2 col + (1: -delta) (base_binary_edge.hpp:157-170): its and the
// zeroing of DR do not reach it, and pop drops them
SE3_HD void perturbed_pose(const double* tab, const double* st, const double* Rwb0, const double* Rcb, const double* tcb, int k,
                           double* Rcw, double* tcw) {
    const double delta = 1e-9;                                                 // :147
    const int col = k >> 1;
    const double step = (k & 1) ? -delta : delta;
    const double* dR = tab + 9 * (col == 0 ? (k & 1) : 2);
    double DR[9], twb[3];
    mul33(dR, st + kDR, DR);
    for (int c = 0; c < 3; c++) twb[c] = st[kTwb + c] + (col == c + 1 ? step : 0.0);
    camera_pose(DR, twb, Rwb0, Rcb, tcb, Rcw, tcw);
}

// Error vector `which` of an edge's linearisation (kErrors of them).  s0 / s1: the two estimates; c0 / c1: the vertices' constants
// as three pointers {Rwb0, Rcb, tcb}
SE3_HD void edge_error_variant(const double* tab, const double* meas, const double* s0, const double* const* c0, const double* s1,
                               const double* const* c1, int which, double* e) {
    if (which == 0) { edge_error(s0 + kRcw, s0 + kTcw, s1 + kRcw, s1 + kTcw, meas, e); return; }
    double R[9], t[3];
    if (which < 9) {
        perturbed_pose(tab, s0, c0[0], c0[1], c0[2], which - 1, R, t);
        edge_error(R, t, s1 + kRcw, s1 + kTcw, meas, e);
    } else {
        perturbed_pose(tab, s1, c1[0], c1[1], c1[2], which - 9, R, t);
        edge_error(s0 + kRcw, s0 + kTcw, R, t, meas, e);
    }
}

// _jacobianOplusX.col(col) = scalar * (error(+delta) - error(-delta)) (base_binary_edge.hpp:162-172), entry d; err: [kErrors][6]
SE3_HD double jacobian_entry(const double* err, int side, int d, int col) {
    const double scalar = 1.0 / (2 * 1e-9);                                    // :147-148
    const int plus = 1 + 8 * side + 2 * col;
    return scalar * (err[6 * plus + d] - err[6 * (plus + 1) + d]);
}

// sum over d of (X[d][a] Omega_d) Y[d][c]: an entry of (X^T Omega) Y (base_binary_edge.hpp:77-89); X, Y: [6][4]
SE3_HD double weighted_dot(const double* X, int a, const double* Y, int c) {
    double t = (X[a] * information(0)) * Y[c];
    for (int d = 1; d < 6; d++) t += (X[4 * d + a] * information(d)) * Y[4 * d + c];
    return t;
}

// Plane q of constructQuadraticForm's terms; J: [2][6][4] as J[side][d][col], e: the base error.  A fixed end's planes are never
// asked for.
SE3_HD double quadratic_term(const double* J, const double* e, int q) {
    const double *A = J, *B = J + 24;
    if (q < kHab) {
        const double* M = q < kHbb ? A : B;
        int k = q < kHbb ? q : q - kHbb, a = 0;
        while (k >= 4 - a) { k -= 4 - a; a++; }
        return weighted_dot(M, a, M, a + k);
    }
    if (q < kBa) return weighted_dot(A, (q - kHab) / 4, B, (q - kHab) % 4);
    const double* M = q < kBb ? A : B;
    const int a = q < kBb ? q - kBa : q - kBb;
    double t = M[a] * -(information(0) * e[0]);                                // omega_r = -omega * _error (:74)
    for (int d = 1; d < 6; d++) t += M[4 * d + a] * -(information(d) * e[d]);
    return t;
}

// position of (r, c), r <= c, in a row-major upper triangle of a 4x4
SE3_HD int upper4(int r, int c) { return r * 4 - (r * (r - 1)) / 2 + (c - r); }

// computeLambdaInit (optimization_algorithm_levenberg.cpp:172-186) without a user value: tau = 1e-5 times the largest |H(j, j)|
SE3_HD double lambda_init(double max_diagonal) { return 1e-5 * max_diagonal; }

}  // namespace eg4
}  // namespace msorb
