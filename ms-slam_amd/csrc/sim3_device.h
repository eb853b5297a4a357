// Sim3Solver::ComputeSim3 (src/Sim3Solver.cc:390-491) and one correspondence of Sim3Solver::CheckInliers (:494-518) for two pinhole
// cameras.  One statement of the arithmetic for the device (sim3_hypotheses_kernel, sim3.hip) and the host: every float operation
// is a single correctly rounded IEEE operation in the reference's statement order, sums taken left to right, nothing contracted
// (the np_* operators of new_points_device.h).  DESIGN.md section 12 lists, line by line, what the reference leaves to Eigen and
// libm and what is fixed here instead.
#pragma once
#include "new_points_device.h"

namespace msorb {

constexpr int kSim3MaxSweeps = 16;   // cyclic Jacobi on a symmetric 4x4 in float: the test scenes need 3-5 rotating sweeps

struct Sim3Transform {
    float s;        // ms12i
    float R[9];     // mR12i, row major
    float t[3];     // mt12i
    float sR[9];    // mT12i.block<3,3>(0,0) (:477)
    float sRinv[9]; // mT21i.block<3,3>(0,0) (:484)
    float tinv[3];  // mT21i.block<3,1>(0,3) (:489)
};

// The eigenvector of the symmetric 4x4 matrix A (row major) for its largest eigenvalue (:432-441 take it from
// Eigen::EigenSolver<Matrix4f>, a general solver whose bits are not pinned): cyclic Jacobi, the pairs (p, q) in the order
// (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), a pair rotated when |A(p,q)| > max(FLT_MIN, 2 eps max|A(i,i)|), with
//   tau = (A(q,q) - A(p,p)) / (2 A(p,q)),  t = 1 / (tau +- sqrt(tau^2 + 1)) (the sign of tau),  c = 1 / sqrt(t^2 + 1),  s = t c,
// sweeps until one passes without a rotation or kSim3MaxSweeps are done.  The eigenvalue is the first maximum of the diagonal
// (maxCoeff, :439); the vector's sign is whatever the rotations leave: q and -q are one rotation.  An A whose entries are all
// infinite (or all NaN) rotates nothing (every comparison is false) and returns the first unit vector.  A single NaN or infinity
// does not stop the pairs it is not in (np_max keeps a NaN out of max_diag) and spreads through the rows they rotate; q is then
// whatever column the comparisons, false against a NaN, leave as the first maximum, and may be finite.
NP_HD void sim3_largest_eigenvector(const float* A, float* q) {
    const float tiny = 1.17549435e-38f, precision = 2.384185791015625e-07f;   // FLT_MIN, 2 * FLT_EPSILON
    float W[4][4], V[4][4];
NP_UNROLL
    for (int i = 0; i < 4; i++)
NP_UNROLL
        for (int j = 0; j < 4; j++) { W[i][j] = A[4 * i + j]; V[i][j] = i == j ? 1.0f : 0.0f; }
    float max_diag = np_max(np_max(np_abs(W[0][0]), np_abs(W[1][1])), np_max(np_abs(W[2][2]), np_abs(W[3][3])));
    for (int sweep = 0; sweep < kSim3MaxSweeps; sweep++) {
        bool finished = true;
NP_UNROLL
        for (int p = 0; p < 3; p++)
NP_UNROLL
            for (int r = p + 1; r < 4; r++) {
                const float apq = W[p][r];
                const float thr = np_max(tiny, np_mul(precision, max_diag));
                if (!(np_abs(apq) > thr)) continue;
                finished = false;
                const float app = W[p][p], aqq = W[r][r];
                const float tau = np_div(np_sub(aqq, app), np_mul(2.0f, apq));
                const float w = np_sqrt(np_add(np_mul(tau, tau), 1.0f));
                const float t = tau >= 0.0f ? np_div(1.0f, np_add(tau, w)) : np_div(1.0f, np_sub(tau, w));
                const float c = np_div(1.0f, np_sqrt(np_add(np_mul(t, t), 1.0f)));
                const float s = np_mul(t, c);
                const float tapq = np_mul(t, apq);
                W[p][p] = np_sub(app, tapq);
                W[r][r] = np_add(aqq, tapq);
                W[p][r] = 0.0f;
                W[r][p] = 0.0f;
NP_UNROLL
                for (int k = 0; k < 4; k++) {
                    if (k != p && k != r) {
                        const float akp = W[k][p], akq = W[k][r];
                        const float nkp = np_axmby(c, akp, s, akq), nkq = np_axpby(s, akp, c, akq);
                        W[k][p] = nkp; W[p][k] = nkp;
                        W[k][r] = nkq; W[r][k] = nkq;
                    }
                    const float vkp = V[k][p], vkq = V[k][r];
                    V[k][p] = np_axmby(c, vkp, s, vkq);
                    V[k][r] = np_axpby(s, vkp, c, vkq);
                }
                max_diag = np_max(max_diag, np_max(np_abs(W[p][p]), np_abs(W[r][r])));
            }
        if (finished) break;
    }
    int best = 0;
    float ev = W[0][0];
NP_UNROLL
    for (int i = 1; i < 4; i++)
        if (W[i][i] > ev) { ev = W[i][i]; best = i; }
NP_UNROLL
    for (int i = 0; i < 4; i++) q[i] = best == 0 ? V[i][0] : best == 1 ? V[i][1] : best == 2 ? V[i][2] : V[i][3];
}

// The rotation matrix of the quaternion q = (w, x, y, z) / |q| (:441-447 reach it through atan2 in double and SO3f::exp of
// 2 ang vec / (|vec| + 1e-12); this is the same rotation in algebraic form, off by rounding only).
NP_HD void sim3_rotation_of_quaternion(const float* q, float* R) {
    const float n = np_sqrt(np_add(np_add(np_add(np_mul(q[0], q[0]), np_mul(q[1], q[1])), np_mul(q[2], q[2])), np_mul(q[3], q[3])));
    const float w = np_div(q[0], n), x = np_div(q[1], n), y = np_div(q[2], n), z = np_div(q[3], n);
    const float tx = np_mul(2.0f, x), ty = np_mul(2.0f, y), tz = np_mul(2.0f, z);
    const float twx = np_mul(tx, w), twy = np_mul(ty, w), twz = np_mul(tz, w);
    const float txx = np_mul(tx, x), txy = np_mul(ty, x), txz = np_mul(tz, x);
    const float tyy = np_mul(ty, y), tyz = np_mul(tz, y), tzz = np_mul(tz, z);
    R[0] = np_sub(1.0f, np_add(tyy, tzz)); R[1] = np_sub(txy, twz);               R[2] = np_add(txz, twy);
    R[3] = np_add(txy, twz);               R[4] = np_sub(1.0f, np_add(txx, tzz)); R[5] = np_sub(tyz, twx);
    R[6] = np_sub(txz, twy);               R[7] = np_add(tyz, twx);               R[8] = np_sub(1.0f, np_add(txx, tyy));
}

// ComputeSim3 (:390-491).  P1 / P2: the three points of each set, point i at [3 i, 3 i + 3) (the columns of P3Dc1i / P3Dc2i).
NP_HD void sim3_compute(const float* P1, const float* P2, bool fix_scale, Sim3Transform& T) {
    // :381-387 ComputeCentroid: the row sums left to right, divided by 3
    float O1[3], O2[3], Pr1[9], Pr2[9];   // Pr: point i at [3 i, 3 i + 3)
NP_UNROLL
    for (int r = 0; r < 3; r++) {
        O1[r] = np_div(np_add(np_add(P1[r], P1[3 + r]), P1[6 + r]), 3.0f);
        O2[r] = np_div(np_add(np_add(P2[r], P2[3 + r]), P2[6 + r]), 3.0f);
    }
NP_UNROLL
    for (int i = 0; i < 3; i++)
NP_UNROLL
        for (int r = 0; r < 3; r++) { Pr1[3 * i + r] = np_sub(P1[3 * i + r], O1[r]); Pr2[3 * i + r] = np_sub(P2[3 * i + r], O2[r]); }
    // :407 M = Pr2 * Pr1^T: M(r, c) = sum over the points of Pr2(r, i) Pr1(c, i)
    float M[3][3];
NP_UNROLL
    for (int r = 0; r < 3; r++)
NP_UNROLL
        for (int c = 0; c < 3; c++) M[r][c] = np_dot3(Pr2[r], Pr2[3 + r], Pr2[6 + r], Pr1[c], Pr1[3 + c], Pr1[6 + c]);
    // :414-428: every right-hand side is a float expression; the double locals hold it exactly and Matrix4f gets the same float back
    const float N11 = np_add(np_add(M[0][0], M[1][1]), M[2][2]);
    const float N12 = np_sub(M[1][2], M[2][1]);
    const float N13 = np_sub(M[2][0], M[0][2]);
    const float N14 = np_sub(M[0][1], M[1][0]);
    const float N22 = np_sub(np_sub(M[0][0], M[1][1]), M[2][2]);
    const float N23 = np_add(M[0][1], M[1][0]);
    const float N24 = np_add(M[2][0], M[0][2]);
    const float N33 = np_sub(np_add(-M[0][0], M[1][1]), M[2][2]);
    const float N34 = np_add(M[1][2], M[2][1]);
    const float N44 = np_add(np_sub(-M[0][0], M[1][1]), M[2][2]);
    const float N[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    float q[4];
    sim3_largest_eigenvector(N, q);
    sim3_rotation_of_quaternion(q, T.R);
    // :450 P3 = mR12i * Pr2
    float P3[9];
NP_UNROLL
    for (int i = 0; i < 3; i++)
NP_UNROLL
        for (int r = 0; r < 3; r++) P3[3 * i + r] = np_dot3(T.R[3 * r], T.R[3 * r + 1], T.R[3 * r + 2], Pr2[3 * i], Pr2[3 * i + 1], Pr2[3 * i + 2]);
    // :457-464: nom and den are float sums (over the points, inside a point over x, y, z) widened to double; the quotient is a
    // double division narrowed to the float ms12i
    if (!fix_scale) {
        float nom = 0.0f, den = 0.0f;
NP_UNROLL
        for (int k = 0; k < 9; k++) {
            const float a = np_mul(Pr1[k], P3[k]), b = np_mul(P3[k], P3[k]);
            nom = k == 0 ? a : np_add(nom, a);
            den = k == 0 ? b : np_add(den, b);
        }
        T.s = (float)np_ddiv((double)nom, (double)den);
    } else {
        T.s = 1.0f;
    }
    // :477 sR = ms12i * mR12i, :470 mt12i = O1 - sR * O2
NP_UNROLL
    for (int k = 0; k < 9; k++) T.sR[k] = np_mul(T.s, T.R[k]);
NP_UNROLL
    for (int r = 0; r < 3; r++) T.t[r] = np_sub(O1[r], np_dot3(T.sR[3 * r], T.sR[3 * r + 1], T.sR[3 * r + 2], O2[0], O2[1], O2[2]));
    // :484 (1.0 / ms12i) is a double division; Eigen narrows the factor to the matrix's float before the product
    const float inv = (float)np_ddiv(1.0, (double)T.s);
NP_UNROLL
    for (int r = 0; r < 3; r++)
NP_UNROLL
        for (int c = 0; c < 3; c++) T.sRinv[3 * r + c] = np_mul(inv, T.R[3 * c + r]);
    // :489 tinv = -sRinv * mt12i (negating the factors or the sum gives the same bits)
NP_UNROLL
    for (int r = 0; r < 3; r++) T.tinv[r] = -np_dot3(T.sRinv[3 * r], T.sRinv[3 * r + 1], T.sRinv[3 * r + 2], T.t[0], T.t[1], T.t[2]);
}

// Pinhole::project of the float vector (src/CameraModels/Pinhole.cpp:43-49); cam = fx, fy, cx, cy
NP_HD void sim3_project(const float* cam, float x, float y, float z, float& u, float& v) {
    u = np_add(np_div(np_mul(cam[0], x), z), cam[2]);
    v = np_add(np_div(np_mul(cam[1], y), z), cam[3]);
}

// One i of CheckInliers (:502-517) with Project (:540-554) and FromCameraToImage (:556-566) for that correspondence.
NP_HD bool sim3_is_inlier(const Sim3Transform& T, const float* cam1, const float* cam2, const float* X1, const float* X2, float max_err1,
                          float max_err2) {
    float p1u, p1v, p2u, p2v, a_u, a_v, b_u, b_v;
    sim3_project(cam1, X1[0], X1[1], X1[2], p1u, p1v);   // mvP1im1[i]
    sim3_project(cam2, X2[0], X2[1], X2[2], p2u, p2v);   // mvP2im2[i]
    float c[3];
NP_UNROLL
    for (int r = 0; r < 3; r++) c[r] = np_add(np_dot3(T.sR[3 * r], T.sR[3 * r + 1], T.sR[3 * r + 2], X2[0], X2[1], X2[2]), T.t[r]);
    sim3_project(cam1, c[0], c[1], c[2], a_u, a_v);      // vP2im1[i]
NP_UNROLL
    for (int r = 0; r < 3; r++) c[r] = np_add(np_dot3(T.sRinv[3 * r], T.sRinv[3 * r + 1], T.sRinv[3 * r + 2], X1[0], X1[1], X1[2]), T.tinv[r]);
    sim3_project(cam2, c[0], c[1], c[2], b_u, b_v);      // vP1im2[i]
    const float d1u = np_sub(p1u, a_u), d1v = np_sub(p1v, a_v), d2u = np_sub(b_u, p2u), d2v = np_sub(b_v, p2v);
    const float err1 = np_add(np_mul(d1u, d1u), np_mul(d1v, d1v)), err2 = np_add(np_mul(d2u, d2u), np_mul(d2v, d2v));
    return err1 < max_err1 && err2 < max_err2;
}

}  // namespace msorb
