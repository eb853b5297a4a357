// Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:4422-4779) and PoseInertialOptimizationLastFrame (:4781-5172)
// after their gathering loops, for pinhole mono / stereo frames without a second camera: the graph of EdgeMonoOnlyPose /
// EdgeStereoOnlyPose (include/G2oTypes.h:390-493, src/G2oTypes.cc:375-490), EdgeInertial (G2oTypes.cc:492-594), EdgeGyroRW /
// EdgeAccRW (G2oTypes.h:635-704) and, against the previous frame, EdgePriorPoseImu (G2oTypes.cc:720-760), over ImuCamPose
// (G2oTypes.cc:73-119, :192-220); Gauss-Newton (optimization_algorithm_gauss_newton.cpp:50-93 under sparse_optimizer.cpp:354-419),
// the quadratic form of a BaseMultiEdge (base_multi_edge.hpp:171-222), the four classifications, the recovery arm, the Hessians of
// :4743-4773 / :5120-5162, Marginalize (:2975-3048) and ConstraintPoseImu's constructor (G2oTypes.h:711-722).  One statement of the
// arithmetic for the device (pose_inertial.hip) and the host (tests/pose_inertial_main.cc), as inertial_device.h is: plain
// arithmetic in the order the reference writes it, a product of small matrices the row-by-column sum left to right, nothing
// contracted (-ffp-contract=off).  DESIGN.md section 20.
//
// The routine is a template over
//   an executor:  ex.tid(), ex.stride(), ex.barrier(), ex.sum(v, n) (n <= kSums) as inertial_device.h describes them, and
//                 ex.leads(k): this executor walks the k-th serial job of a pass (host: always; device: lane 0 of wavefront k,
//                 so the inertial and the prior edge are evaluated side by side);
//   the edges:    obs.each(f) calls f(const Ob&, double& chi2, uint8_t& level, int index) for this executor's visual edges in
//                 ascending index; chi2 and level are the edge's state between the passes (zero at the start).
// and works in a Shared block (LDS on the device) that holds the multi-edges entry by entry: a leader evaluates the
// 3x3 blocks of the inertial edge, another those of the prior edge, every form after that (A^T omega, then A^T omega B, then the L D L^T's trailing
// update) is one executor per entry, each the same row-by-column sum whoever computes it.
//
// Unknowns in the order of the vertex ids: the frame's pose (0-5), velocity (6-8), gyro bias (9-11), acc bias (12-14), then in
// form 1 the previous frame's in the same order (15-29).
#pragma once
#include "inertial_device.h"

namespace msorb {
namespace pinert {

using eg4::dot3;
using eg4::exp_so3;
using eg4::log_so3;
using eg4::mul33;
using eg4::mul3v;
using eg4::normalize_rotation;

constexpr int kSums = 27;          // the pose block of the visual edges: 21 (upper triangle, row major) + 6 (b)
constexpr int kJc = 24;            // EdgeInertial's columns as GetHessian orders them: P1 6, V1 3, G1 3, A1 3, P2 6, V2 3
constexpr int kMaxN = 30;

struct Ob { float x, y, ur, w, X, Y, Z; int close; };   // one visual edge as the reference holds it before the widening
struct Cam { double fx, fy, cx, cy, bf; };

// ImuCamPose of one camera (G2oTypes.cc:73-119): Rcw / tcw are members of their own
struct PoseEst { double Rwb[9], twb[3], Rcw[9], tcw[3]; int its; };
struct Vertices { PoseEst P; double v[3], bg[3], ba[3]; };

struct Shared {
    double J[9 * kJc], AtO[kJc * 9], e[9], Oe[9];          // EdgeInertial: the Jacobian, J^T omega, the error, omega e
    double Jp[15 * 15], AtOp[15 * 15], ep[15], Oep[15];    // EdgePriorPoseImu
    double rw[12];                                         // omega e of EdgeGyroRW, EdgeAccRW (3 + 3), their errors (3 + 3)
    double rho1p;                                          // the prior's robust weight
    double Vs[kSums];                                      // the visual edges' sums, where the system's entries read them
    double H[kMaxN * kMaxN], b[kMaxN], x[kMaxN];           // the system: upper triangle A, then L below the diagonal, D on it
};

// ---- ImuCamPose

SE3_HD void camera_from_body(PoseEst& P, const double* Rcb, const double* tcb) {   // G2oTypes.cc:211-218
    double Rbw[9], tbw[3], t[3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Rbw[3 * r + c] = P.Rwb[3 * c + r];
    mul3v(Rbw, P.twb, t);
    for (int k = 0; k < 3; k++) tbw[k] = -t[k];                                     // (-Rbw) twb
    mul33(Rcb, Rbw, P.Rcw);
    mul3v(Rcb, tbw, t);
    for (int k = 0; k < 3; k++) P.tcw[k] = t[k] + tcb[k];
}

// ImuCamPose::Update (G2oTypes.cc:192-220): twb with the old Rwb, NormalizeRotation on every third update of this estimate
SE3_HD void pose_update(PoseEst& P, const double* u, const double* Rcb, const double* tcb) {
    double t[3], E[9], R[9];
    mul3v(P.Rwb, u + 3, t);
    for (int k = 0; k < 3; k++) P.twb[k] += t[k];
    exp_so3(u[0], u[1], u[2], E);
    mul33(P.Rwb, E, R);
    P.its++;
    if (P.its >= 3) {
        normalize_rotation(R, P.Rwb);
        P.its = 0;
    } else {
        for (int q = 0; q < 9; q++) P.Rwb[q] = R[q];
    }
    camera_from_body(P, Rcb, tcb);
}

SE3_HD void vertices_update(Vertices& V, const double* u, const double* Rcb, const double* tcb) {
    pose_update(V.P, u, Rcb, tcb);
    for (int k = 0; k < 3; k++) { V.v[k] += u[6 + k]; V.bg[k] += u[9 + k]; V.ba[k] += u[12 + k]; }
}

SE3_HD void vertices_init(Vertices& V, const msorb_pose_inertial_state& s) {
    for (int q = 0; q < 9; q++) V.P.Rwb[q] = s.Rwb[q];
    for (int k = 0; k < 3; k++) { V.P.twb[k] = s.twb[k]; V.v[k] = s.v[k]; V.bg[k] = s.bg[k]; V.ba[k] = s.ba[k]; }
    V.P.its = 0;
}

// ---- the visual edges

// computeError (G2oTypes.h:401-405 with ImuCamPose::Project, :477-481 with ProjectStereo, G2oTypes.cc:170-185; Pinhole::project,
// Pinhole.cpp:35-41) -> e[3] (e[2] = 0 for a mono edge), Xc, and chi2() = e . (Omega e) (base_edge.h:60)
SE3_HD double visual_error(const PoseEst& P, const Cam& c, const Ob& o, double* e, double* Xc) {
    const double Xw[3] = {(double)o.X, (double)o.Y, (double)o.Z};
    double t[3];
    mul3v(P.Rcw, Xw, t);
    for (int k = 0; k < 3; k++) Xc[k] = t[k] + P.tcw[k];
    const double w = (double)o.w;
    const double p0 = (c.fx * Xc[0]) / Xc[2] + c.cx, p1 = (c.fy * Xc[1]) / Xc[2] + c.cy;
    e[0] = (double)o.x - p0;
    e[1] = (double)o.y - p1;
    if (o.ur >= 0) {
        const double invZ = 1 / Xc[2];
        e[2] = (double)o.ur - (p0 - c.bf * invZ);
        return (e[0] * (w * e[0]) + e[1] * (w * e[1])) + e[2] * (w * e[2]);
    }
    e[2] = 0;
    return e[0] * (w * e[0]) + e[1] * (w * e[1]);
}

// isDepthPositive (G2oTypes.cc:187-190)
SE3_HD bool depth_positive(const PoseEst& P, const Ob& o) {
    return dot3(P.Rcw[6], P.Rcw[7], P.Rcw[8], (double)o.X, (double)o.Y, (double)o.Z) + P.tcw[2] > 0.0;
}

// linearizeOplus (G2oTypes.cc:375-395, :429-454): (proj_jac Rcb) SE3deriv(Xb) with Xb = Rbc Xc + tbc; projectJac is
// Pinhole.cpp:71-81.  Rbc = Rcb^T.
SE3_HD void visual_jacobian(const Cam& c, bool stereo, const double* Xc, const double* Rcb, const double* tbc, double (*J)[6]) {
    double Xb[3], M[9];
    for (int r = 0; r < 3; r++) Xb[r] = dot3(Rcb[r], Rcb[3 + r], Rcb[6 + r], Xc[0], Xc[1], Xc[2]) + tbc[r];
    const double zz = Xc[2] * Xc[2];
    double pj[9] = {c.fx / Xc[2], 0.0, (-c.fx * Xc[0]) / zz, 0.0, c.fy / Xc[2], (-c.fy * Xc[1]) / zz, 0.0, 0.0, 0.0};
    if (stereo) {
        const double inv_z2 = 1.0 / zz;
        pj[6] = pj[0]; pj[7] = pj[1]; pj[8] = pj[2] + c.bf * inv_z2;
    }
    mul33(pj, Rcb, M);
    const double x = Xb[0], y = Xb[1], z = Xb[2];
    for (int r = 0; r < 3; r++) {
        const double m0 = M[3 * r], m1 = M[3 * r + 1], m2 = M[3 * r + 2];
        J[r][0] = dot3(m0, m1, m2, 0.0, -z, y);
        J[r][1] = dot3(m0, m1, m2, z, 0.0, -x);
        J[r][2] = dot3(m0, m1, m2, -y, x, 0.0);
        J[r][3] = dot3(m0, m1, m2, 1.0, 0.0, 0.0);
        J[r][4] = dot3(m0, m1, m2, 0.0, 1.0, 0.0);
        J[r][5] = dot3(m0, m1, m2, 0.0, 0.0, 1.0);
    }
}

// one edge's A^T (w Omega) A into S[0, 21) and, with e, -(A^T (w Omega) e) into S[21, 27) (base_unary_edge.hpp:43-72)
SE3_HD void visual_add(const double (*J)[6], bool stereo, double w, double rho1, const double* e, double* S) {
    const double wr = rho1 * w;
    int k = 0;
    for (int a = 0; a < 6; a++) {
        for (int c = a; c < 6; c++, k++) {
            double t = (J[0][a] * wr) * J[0][c] + (J[1][a] * wr) * J[1][c];
            if (stereo) t += (J[2][a] * wr) * J[2][c];
            S[k] += t;
        }
        if (e) {
            double t = ((rho1 * J[0][a]) * w) * e[0] + ((rho1 * J[1][a]) * w) * e[1];
            if (stereo) t += ((rho1 * J[2][a]) * w) * e[2];
            S[21 + a] -= t;
        }
    }
}

// ---- EdgeInertial, EdgeGyroRW, EdgeAccRW, EdgePriorPoseImu: the leader's part

SE3_HD void put33(double* M, int ld, int r0, int c0, const double* B, double s) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) M[(r0 + r) * ld + c0 + c] = s * B[3 * r + c];
}
SE3_HD void hat(const double* v, double* W) {
    W[0] = 0.0; W[1] = -v[2]; W[2] = v[1];
    W[3] = v[2]; W[4] = 0.0; W[5] = -v[0];
    W[6] = -v[1]; W[7] = v[0]; W[8] = 0.0;
}

// EdgeInertial::computeError (G2oTypes.cc:514-534) and linearizeOplus (:536-594) at one estimate: 1 = the other end, 2 = the
// frame.  The bias of GetDelta* is the other end's estimate narrowed to float; inertial::edge_error is this error with Rwg = I,
// s = 1.  Of one edge `pre` with its information `info`: writes e, Oe = Omega e and, with `jac`, the non-zero blocks of the
// caller's J [9][kJc] (the rest stays zero).  LocalInertialBA's edges (local_inertial_ba_device.h) share it with the two
// tracking forms, whose inertial_terms below hands it the problem's edge and the Shared block.
SE3_HD void inertial_edge_terms(const msorb_inertial_edge& pre, const double* info, const Vertices& F, const Vertices& O, bool jac,
                                double* SJ, double* Se, double* SOe) {
    inertial::Globals G;
    for (int q = 0; q < 9; q++) G.Rwg[q] = q % 4 == 0 ? 1.0 : 0.0;
    G.scale = 1.0;
    msorb_inertial_keyframe k1, k2;
    for (int q = 0; q < 9; q++) { k1.Rwb[q] = O.P.Rwb[q]; k2.Rwb[q] = F.P.Rwb[q]; }
    for (int k = 0; k < 3; k++) { k1.twb[k] = O.P.twb[k]; k2.twb[k] = F.P.twb[k]; G.bg[k] = O.bg[k]; G.ba[k] = O.ba[k]; }
    double e[9], Oe[9];
    inertial::EdgeTerms T;
    inertial::edge_error(pre, k1, k2, O.v, F.v, G, e, T);
    inertial::edge_chi2(info, e, Oe);
    for (int k = 0; k < 9; k++) { Se[k] = e[k]; SOe[k] = Oe[k]; }
    if (!jac) return;
    const double dt = T.dt, g[3] = {0.0, 0.0, -inertial::gravity_value()};
    double invJr[9], nInv[9], A[9], B[9], W[9], tv[3], tp[3], r[3], Rwb2t[9], eRt[9], RJ[9], JRg[9], w[3];
    inertial::inverse_right_jacobian_so3(e[0], e[1], e[2], invJr);                 // :556
    for (int q = 0; q < 9; q++) { nInv[q] = -invJr[q]; JRg[q] = (double)pre.JRg[q]; }
    for (int r_ = 0; r_ < 3; r_++)
        for (int c = 0; c < 3; c++) { Rwb2t[3 * r_ + c] = F.P.Rwb[3 * c + r_]; eRt[3 * r_ + c] = T.eR[3 * c + r_]; }
    mul33(nInv, Rwb2t, A);                                                         // :561
    mul33(A, O.P.Rwb, B);
    put33(SJ, kJc, 0, 0, B, 1.0);
    for (int k = 0; k < 3; k++) {
        tv[k] = T.dv[k] - g[k] * dt;                                               // :562
        tp[k] = T.dp[k] - ((0.5 * g[k]) * dt) * dt;                                // :563-564
    }
    mul3v(T.Rbw1, tv, r);
    hat(r, W);
    put33(SJ, kJc, 3, 0, W, 1.0);
    mul3v(T.Rbw1, tp, r);
    hat(r, W);
    put33(SJ, kJc, 6, 0, W, 1.0);
    for (int k = 0; k < 3; k++) SJ[(6 + k) * kJc + 3 + k] = -1.0;                 // :566
    put33(SJ, kJc, 3, 6, T.Rbw1, -1.0);                                           // :570
    for (int q = 0; q < 9; q++) A[q] = -T.Rbw1[q] * dt;                            // :571
    put33(SJ, kJc, 6, 6, A, 1.0);
    mul3v(JRg, T.dbg, w);                                                          // :575: ((-invJr eR^T) RJ) JRg
    inertial::right_jacobian_so3(w[0], w[1], w[2], RJ);
    mul33(nInv, eRt, A);
    mul33(A, RJ, B);
    mul33(B, JRg, A);
    put33(SJ, kJc, 0, 9, A, 1.0);
    for (int r_ = 0; r_ < 3; r_++)
        for (int c = 0; c < 3; c++) {
            SJ[(3 + r_) * kJc + 9 + c] = -(double)pre.JVg[3 * r_ + c];          // :576
            SJ[(6 + r_) * kJc + 9 + c] = -(double)pre.JPg[3 * r_ + c];          // :577
            SJ[(3 + r_) * kJc + 12 + c] = -(double)pre.JVa[3 * r_ + c];         // :581
            SJ[(6 + r_) * kJc + 12 + c] = -(double)pre.JPa[3 * r_ + c];         // :582
        }
    put33(SJ, kJc, 0, 15, invJr, 1.0);                                            // :587
    mul33(T.Rbw1, F.P.Rwb, A);                                                     // :589
    put33(SJ, kJc, 6, 18, A, 1.0);
    put33(SJ, kJc, 3, 21, T.Rbw1, 1.0);                                           // :593
}
INERTIAL_OUT_OF_LINE SE3_HD void inertial_terms(const msorb_pose_inertial_problem& P, const Vertices& F, const Vertices& O, bool jac,
                                                Shared& S) {
    inertial_edge_terms(P.pre, P.pre.info, F, O, jac, S.J, S.e, S.Oe);
}

// EdgeGyroRW / EdgeAccRW computeError (G2oTypes.h:645-649, :681-685): S.rw = [Og eg | Oa ea | eg | ea]
SE3_HD void random_walk_terms(const msorb_pose_inertial_problem& P, const Vertices& F, const Vertices& O, Shared& S) {
    double eg[3], ea[3], t[3];
    for (int k = 0; k < 3; k++) { eg[k] = F.bg[k] - O.bg[k]; ea[k] = F.ba[k] - O.ba[k]; }
    mul3v(P.info_gyro, eg, t);
    for (int k = 0; k < 3; k++) { S.rw[k] = t[k]; S.rw[6 + k] = eg[k]; }
    mul3v(P.info_acc, ea, t);
    for (int k = 0; k < 3; k++) { S.rw[3 + k] = t[k]; S.rw[9 + k] = ea[k]; }
}

// EdgePriorPoseImu::computeError (G2oTypes.cc:731-745) and linearizeOplus (:747-760) on the other end's vertices; chi2 and the
// Huber weight of delta 5 (Optimizer.cc:4992-4994).  Writes S.ep, S.Oep, S.rho1p and the non-zero blocks of S.Jp.
INERTIAL_OUT_OF_LINE SE3_HD void prior_terms(const msorb_pose_inertial_problem& P, const Vertices& O, bool robust, bool jac, Shared& S) {
    double Rt[9], A[9], e[15], d[3], t[3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Rt[3 * r + c] = P.prior.Rwb[3 * c + r];
    mul33(Rt, O.P.Rwb, A);
    log_so3(A, e);
    for (int k = 0; k < 3; k++) d[k] = O.P.twb[k] - P.prior.twb[k];
    mul3v(Rt, d, t);
    for (int k = 0; k < 3; k++) {
        e[3 + k] = t[k];
        e[6 + k] = O.v[k] - P.prior.v[k];
        e[9 + k] = O.bg[k] - P.prior.bg[k];
        e[12 + k] = O.ba[k] - P.prior.ba[k];
    }
    double chi = 0;
    for (int r = 0; r < 15; r++) {
        double s = P.H[15 * r] * e[0];
        for (int c = 1; c < 15; c++) s += P.H[15 * r + c] * e[c];
        S.Oep[r] = s;
        S.ep[r] = e[r];
        chi = r == 0 ? e[0] * s : chi + e[r] * s;
    }
    double rho0, rho1;
    se3::huber(chi, 5.0, robust, rho0, rho1);
    S.rho1p = rho1;
    if (!jac) return;
    double invJr[9];
    inertial::inverse_right_jacobian_so3(e[0], e[1], e[2], invJr);                 // :752
    put33(S.Jp, 15, 0, 0, invJr, 1.0);
    put33(S.Jp, 15, 3, 3, A, 1.0);                                                 // :753
    for (int k = 6; k < 15; k++) S.Jp[16 * k] = 1.0;                               // :755-759
}

// ---- the system

// the inertial edge's column of unknown u (-1: none): the frame's pose and velocity are its columns 15..23, the other end's
// fifteen its columns 0..14
template <int FORM>
SE3_HD int inertial_col(int u) { return u < 9 ? 15 + u : (FORM == 1 && u >= 15) ? u - 15 : -1; }

SE3_HD int tri6(int a, int b) { return a * 6 - (a * (a - 1)) / 2 + (b - a); }      // upper triangle of a 6x6, row major

// AtO = A^T omega of the inertial edge and, in form 1, of the prior edge with its robust weight on omega (base_edge.h:96-100):
// one executor per entry, the nine / fifteen products left to right
template <int FORM, typename Exec>
SE3_HD void form_AtO(Exec& ex, const msorb_pose_inertial_problem& P, Shared& S, bool weighted) {
    const int total = kJc * 9 + (FORM == 1 ? 225 : 0);
    for (int q = ex.tid(); q < total; q += ex.stride()) {
        if (q < kJc * 9) {
            const int a = q / 9, c = q % 9;
            double t = S.J[a] * P.pre.info[c];
            for (int k = 1; k < 9; k++) t += S.J[k * kJc + a] * P.pre.info[9 * k + c];
            S.AtO[q] = t;
        } else {
            const int p = q - kJc * 9, a = p / 15, c = p % 15;
            double t = 0;
            for (int k = 0; k < 15; k++) {
                const double o = weighted ? S.rho1p * P.H[15 * k + c] : P.H[15 * k + c];
                const double m = S.Jp[k * 15 + a] * o;
                t = k == 0 ? m : t + m;
            }
            S.AtOp[p] = t;
        }
    }
}

// entry (r, c) of the edges' A^T omega B, in the order inertial, gyro random walk, acc random walk, prior (unknowns r, c)
template <int FORM>
SE3_HD double multi_edge_entry(const msorb_pose_inertial_problem& P, const Shared& S, int r, int c) {
    double v = 0;
    const int a = inertial_col<FORM>(r), b = inertial_col<FORM>(c);
    if (a >= 0 && b >= 0) {
        double t = S.AtO[a * 9] * S.J[b];
        for (int k = 1; k < 9; k++) t += S.AtO[a * 9 + k] * S.J[k * kJc + b];
        v = t;
    }
    // J = [-I | I] on (other, frame): omega on both diagonal blocks, -omega between them (G2oTypes.h:651-662)
    const int rr = r % 15, cc = c % 15;
    const bool same = (r < 15) == (c < 15);
    if (FORM == 1 || (r < 15 && c < 15)) {
        if (rr >= 9 && rr < 12 && cc >= 9 && cc < 12) v += same ? P.info_gyro[3 * (rr - 9) + (cc - 9)] : -P.info_gyro[3 * (rr - 9) + (cc - 9)];
        if (rr >= 12 && cc >= 12) v += same ? P.info_acc[3 * (rr - 12) + (cc - 12)] : -P.info_acc[3 * (rr - 12) + (cc - 12)];
    }
    if (FORM == 1 && r >= 15 && c >= 15) {
        double t = S.AtOp[(r - 15) * 15] * S.Jp[c - 15];
        for (int k = 1; k < 15; k++) t += S.AtOp[(r - 15) * 15 + k] * S.Jp[k * 15 + (c - 15)];
        v += t;
    }
    return v;
}

// entry r of the edges' A^T (-(omega e)), same order
template <int FORM>
SE3_HD double multi_edge_b(const Shared& S, int r) {
    double v = 0;
    const int a = inertial_col<FORM>(r);
    if (a >= 0) {
        double t = S.J[a] * -S.Oe[0];
        for (int k = 1; k < 9; k++) t += S.J[k * kJc + a] * -S.Oe[k];
        v = t;
    }
    const int rr = r % 15;
    if (rr >= 9) v += r < 15 ? -S.rw[rr - 9] : S.rw[rr - 9];                       // frame: I^T (-(omega e)); other: (-I)^T (-(omega e))
    if (FORM == 1 && r >= 15) {
        double t = S.Jp[r - 15] * -(S.rho1p * S.Oep[0]);
        for (int k = 1; k < 15; k++) t += S.Jp[k * 15 + (r - 15)] * -(S.rho1p * S.Oep[k]);
        v += t;
    }
    return v;
}

// Unpivoted square-root-free L D L^T of S.H (upper triangle, stride N) in place, column by column, b carried as one more column
// (the forward substitution).  The trailing update of column j is one executor per entry (r, c), j < r <= c <= N, each forming
// L(r, j) = A(j, r) / d_j itself; the diagonal's executor stores it below the diagonal.  One barrier per column.  Then
// x_i = y_i / d_i - sum over m > i of L(m, i) x_m, column by column from the last: one executor per row, one barrier per column
// (the executors' common barrier: on the device the workgroup's).  The terms of that sum are therefore subtracted with m
// DESCENDING; the restatement of tests/pose_inertial_cases.py subtracts them with m ascending, a difference of rounding inside D.
// false: a pivot that is not > 0 ("solver failed"); S.x keeps what it held.  Every executor takes the same path.
template <int N, typename Exec>
SE3_HD bool ldlt_solve(Exec& ex, Shared& S) {
    constexpr int W = 32;                                                          // a row's entries side by side: N + 1 <= W
    static_assert(N + 1 <= W, "a row of the system and b fit one stripe");
    for (int j = 0; j < N; j++) {
        const double d = S.H[j * N + j];
        if (!(d > 0)) return false;
        const double rinv = 1.0 / d;
        for (int q = ex.tid(); q < (N - 1 - j) * W; q += ex.stride()) {
            const int r = j + 1 + q / W, c = j + 1 + q % W;
            if (c > N || c < r) continue;
            const double l = S.H[j * N + r] * rinv;
            if (c == N) S.b[r] -= l * S.b[j];
            else S.H[r * N + c] -= l * S.H[j * N + c];
            if (c == r) S.H[r * N + j] = l;
        }
        ex.barrier();
    }
    for (int r = ex.tid(); r < N; r += ex.stride()) S.b[r] = S.b[r] * (1.0 / S.H[r * N + r]);
    ex.barrier();
    for (int i = N - 1; i >= 1; i--) {
        for (int r = ex.tid(); r < i; r += ex.stride()) S.b[r] -= S.H[i * N + r] * S.b[i];
        ex.barrier();
    }
    for (int r = ex.tid(); r < N; r += ex.stride()) S.x[r] = S.b[r];
    ex.barrier();
    return true;
}

// One call.  flags [n]: the outlier flags as the caller's mvbOutlier ends up.  Every executor returns with the same state; the
// leader writes R (H_prior is the host's: finish_prior).
template <int FORM, typename Exec, typename Obs>
SE3_HD void optimize(Exec& ex, Obs& obs, const msorb_pose_inertial_problem& P, Shared& S, uint8_t* flags, msorb_pose_inertial_result& R) {
    constexpr int N = FORM == 1 ? 30 : 15;
    const int n = P.n;
    const Cam cam{(double)P.fx, (double)P.fy, (double)P.cx, (double)P.cy, (double)P.mbf};
    const double d_mono = (double)(float)sqrt(5.991), d_stereo = (double)(float)sqrt(7.815);   // Optimizer.cc:4470-4471
    // :4623-4624 / :4999-5000
    const float chi2_mono[4] = {FORM == 0 ? 12.0f : 5.991f, FORM == 0 ? 7.5f : 5.991f, 5.991f, 5.991f};
    const float chi2_stereo[4] = {15.6f, 9.8f, 7.815f, 7.815f};
    Vertices F, O;
    vertices_init(F, P.frame);
    vertices_init(O, P.other);
    for (int q = 0; q < 9; q++) F.P.Rcw[q] = P.Rcw[q];                             // G2oTypes.cc:95-96
    for (int k = 0; k < 3; k++) F.P.tcw[k] = P.tcw[k];
    camera_from_body(O.P, P.Rcb, P.tcb);                                           // (no edge reads the other end's camera pose)
    for (int q = ex.tid(); q < 9 * kJc; q += ex.stride()) S.J[q] = 0.0;
    for (int q = ex.tid(); q < 225; q += ex.stride()) S.Jp[q] = 0.0;
    for (int q = ex.tid(); q < kMaxN; q += ex.stride()) S.x[q] = 0.0;              // the solver's x starts at zero
    ex.barrier();
    int iterations[4] = {-1, -1, -1, -1}, failed[4] = {0, 0, 0, 0};
    int n_bad = 0, n_inliers = 0;
    const int n_edges = n + (FORM == 1 ? 4 : 3);                                   // optimizer.edges().size()
    for (int it = 0; it < 4; it++) {
        const bool robust = it < 3;                                                // :4669-4670: the kernels come off after round three
        int passes = 0;
        bool ok = true;
        for (int i = 0; i < 10 && ok; i++) {                                       // gauss_newton.cpp:50-93, its[] = 10
            if (ex.leads(0)) {
                inertial_terms(P, F, O, true, S);
                random_walk_terms(P, F, O, S);
            }
            if (FORM == 1 && ex.leads(1)) prior_terms(P, O, true, true, S);        // the prior keeps its kernel on all four rounds
            double V[kSums];
            for (int k = 0; k < kSums; k++) V[k] = 0;
            obs.each([&](const Ob& o, double& chi2, uint8_t& level, int) {
                if (level) return;
                double e[3], Xc[3], J[3][6], rho0, rho1;
                const bool stereo = o.ur >= 0;
                chi2 = visual_error(F.P, cam, o, e, Xc);                           // computeActiveErrors
                se3::huber(chi2, stereo ? d_stereo : d_mono, robust, rho0, rho1);
                visual_jacobian(cam, stereo, Xc, P.Rcb, P.tbc, J);
                visual_add(J, stereo, (double)o.w, rho1, e, V);
            });
            ex.sum(V, kSums);
            if (ex.tid() == 0)
                for (int k = 0; k < kSums; k++) S.Vs[k] = V[k];
            ex.barrier();                                                          // publishes the leader's terms and the sums
            form_AtO<FORM>(ex, P, S, true);
            ex.barrier();
            for (int q = ex.tid(); q < N * (N + 1); q += ex.stride()) {
                const int r = q / (N + 1), c = q % (N + 1);
                if (c == N) S.b[r] = (r < 6 ? S.Vs[21 + r] : 0.0) + multi_edge_b<FORM>(S, r);
                else if (c >= r) S.H[r * N + c] = (c < 6 ? S.Vs[tri6(r, c)] : 0.0) + multi_edge_entry<FORM>(P, S, r, c);
            }
            ex.barrier();
            ok = ldlt_solve<N>(ex, S);
            ex.barrier();
            vertices_update(F, S.x, P.Rcb, P.tcb);                                 // :85: also when the solve failed
            if (FORM == 1) vertices_update(O, S.x + 15, P.Rcb, P.tcb);
            passes++;
            if (!ok) failed[it] = 1;
        }
        iterations[it] = passes;
        // ---- the classification (:4638-4700 / :5013-5074)
        const float thr_mono = chi2_mono[it], thr_close = (float)(1.5 * (double)chi2_mono[it]), thr_stereo = chi2_stereo[it];
        double bad[1] = {0};
        obs.each([&](const Ob& o, double& chi2, uint8_t& level, int) {
            const bool stereo = o.ur >= 0;
            if (level) {                                                           // :4652-4654
                double e[3], Xc[3];
                chi2 = visual_error(F.P, cam, o, e, Xc);
            }
            const float c = (float)chi2;                                           // :4656
            if (stereo) level = c > thr_stereo ? 1 : 0;
            else level = ((c > thr_mono && !o.close) || (o.close && c > thr_close) || !depth_positive(F.P, o)) ? 1 : 0;
            bad[0] += level;
        });
        ex.sum(bad, 1);
        n_bad = (int)bad[0];
        n_inliers = n - n_bad;
        if (n_edges < 10) break;                                                   // :4702
    }
    // ---- the recovery arm (:4709-4733): flags cleared below 18 / 24, never set
    if (n_inliers < 30 && !P.rec_init) {
        double bad[1] = {0};
        obs.each([&](const Ob& o, double& chi2, uint8_t& level, int) {
            double e[3], Xc[3];
            chi2 = visual_error(F.P, cam, o, e, Xc);
            if (chi2 < (double)(o.ur >= 0 ? 24.f : 18.f)) level = 0;
            else bad[0] += 1;
        });
        ex.sum(bad, 1);
        n_bad = (int)bad[0];
    }
    // ---- the Hessian (:4743-4773 / :5120-5162): every GetHessian*() re-linearises at the returned estimate, plain information
    if (ex.leads(0)) inertial_terms(P, F, O, true, S);
    if (FORM == 1 && ex.leads(1)) prior_terms(P, O, false, true, S);
    double V[kSums];
    for (int k = 0; k < kSums; k++) V[k] = 0;
    obs.each([&](const Ob& o, double& chi2, uint8_t& level, int index) {
        flags[index] = level;
        if (level) return;
        double e[3], Xc[3], J[3][6];
        const bool stereo = o.ur >= 0;
        visual_error(F.P, cam, o, e, Xc);
        visual_jacobian(cam, stereo, Xc, P.Rcb, P.tbc, J);
        visual_add(J, stereo, (double)o.w, 1.0, nullptr, V);
    });
    ex.sum(V, 21);
    if (ex.tid() == 0)
        for (int k = 0; k < 21; k++) S.Vs[k] = V[k];
    ex.barrier();
    form_AtO<FORM>(ex, P, S, false);
    ex.barrier();
    // H_raw's row of unknown u: form 1 puts the previous frame first
    for (int q = ex.tid(); q < N * N; q += ex.stride()) {
        const int hr = q / N, hc = q % N;
        const int r = FORM == 1 ? (hr + 15) % 30 : hr, c = FORM == 1 ? (hc + 15) % 30 : hc;
        double v = multi_edge_entry<FORM>(P, S, r, c);
        if (r < 6 && c < 6) v += r <= c ? S.Vs[tri6(r, c)] : S.Vs[tri6(c, r)];
        R.H_raw[q] = v;
    }
    if (ex.tid() == 0) {
        for (int q = 0; q < 9; q++) { R.est.Rwb[q] = F.P.Rwb[q]; R.Rwb_f[q] = (float)F.P.Rwb[q]; }
        for (int k = 0; k < 3; k++) {
            R.est.twb[k] = F.P.twb[k]; R.est.v[k] = F.v[k]; R.est.bg[k] = F.bg[k]; R.est.ba[k] = F.ba[k];
            R.twb_f[k] = (float)F.P.twb[k];                                        // :4736-4737
            R.v_f[k] = (float)F.v[k];
        }
        R.n_initial = n;
        R.n_bad = n_bad;
        R.n_inliers = n_inliers;
        for (int k = 0; k < 4; k++) { R.iterations[k] = iterations[k]; R.solve_failed[k] = failed[k]; }
    }
}

// ---- host functions: Marginalize (Optimizer.cc:2975-3048) and ConstraintPoseImu's constructor (G2oTypes.h:711-722)

// cyclic Jacobi of the symmetric n x n A (n <= 15) as inertial::info_from_covariance runs it: A's diagonal ends as the
// eigenvalues, V's columns as the eigenvectors
inline void jacobi_eig(int n, double (*A)[15], double (*V)[15]) {
    for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) V[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0, diag = 0;
        for (int r = 0; r < n; r++) {
            diag += A[r][r] * A[r][r];
            for (int c = r + 1; c < n; c++) off += A[r][c] * A[r][c];
        }
        if (!(sqrt(off) > 1e-17 * sqrt(diag))) break;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; k++) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; k++) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; k++) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

// out = V f(diag) V^T, the product (V diag) V^T row by column left to right
template <typename F>
inline void recompose15(double (*A)[15], double (*V)[15], double* out, F f) {
    for (int r = 0; r < 15; r++)
        for (int c = 0; c < 15; c++) {
            double t = 0;
            for (int k = 0; k < 15; k++) {
                const double term = (V[r][k] * f(A[k][k])) * V[c][k];
                t = k == 0 ? term : t + term;
            }
            out[15 * r + c] = t;
        }
}

// Marginalize(H, 0, 14) of the 30x30 H_raw, the trailing 15x15: Hc - Hcb pinv(Hb) Hbc.  The SVD's pseudo-inverse of the symmetric
// leading block (singular values <= 1e-6 dropped) is the eigen-decomposition's with the threshold on |lambda|.
// sigma (may be null): the 15 singular values.
inline void marginalize_previous(const double* H30, double* out15, double* sigma = nullptr) {
    static thread_local double A[15][15], V[15][15];
    double inv[225], T[225];
    for (int r = 0; r < 15; r++)
        for (int c = 0; c < 15; c++) A[r][c] = (H30[30 * r + c] + H30[30 * c + r]) / 2;
    jacobi_eig(15, A, V);
    if (sigma) for (int k = 0; k < 15; k++) sigma[k] = fabs(A[k][k]);
    recompose15(A, V, inv, [](double l) { return fabs(l) > 1e-6 ? 1.0 / l : 0.0; });
    for (int r = 0; r < 15; r++)                                                   // (Hcb invHb) Hbc
        for (int c = 0; c < 15; c++) {
            double t = H30[30 * (15 + r)] * inv[c];
            for (int k = 1; k < 15; k++) t += H30[30 * (15 + r) + k] * inv[15 * k + c];
            T[15 * r + c] = t;
        }
    for (int r = 0; r < 15; r++)
        for (int c = 0; c < 15; c++) {
            double t = T[15 * r] * H30[15 + c];
            for (int k = 1; k < 15; k++) t += T[15 * r + k] * H30[30 * k + 15 + c];
            out15[15 * r + c] = H30[30 * (15 + r) + 15 + c] - t;
        }
}

// ConstraintPoseImu's constructor: (H + H) / 2, SelfAdjointEigenSolver (which reads the lower triangle), eigenvalues below 1e-12 to
// zero, V diag V^T
inline void constraint_information(const double* H15, double* out15, double* eigs = nullptr) {
    static thread_local double A[15][15], V[15][15];
    for (int r = 0; r < 15; r++)
        for (int c = 0; c < 15; c++) A[r][c] = r >= c ? (H15[15 * r + c] + H15[15 * r + c]) / 2 : (H15[15 * c + r] + H15[15 * c + r]) / 2;
    jacobi_eig(15, A, V);
    if (eigs) for (int k = 0; k < 15; k++) eigs[k] = A[k][k];
    recompose15(A, V, out15, [](double l) { return l < 1e-12 ? 0.0 : l; });
}

// what the library call does after the read-back: R.H_prior from R.H_raw (form 0 uses 225 of its 900 entries: the rest is zeroed).
// sigma, eigs (may be null): the 15 singular values Marginalize thresholds (form 1) and the 15 eigenvalues the constructor does.
inline void finish_prior(int form, msorb_pose_inertial_result& R, double* sigma = nullptr, double* eigs = nullptr) {
    if (form == 1) {
        double M[225];
        marginalize_previous(R.H_raw, M, sigma);
        constraint_information(M, R.H_prior, eigs);
    } else {
        for (int q = 225; q < 900; q++) R.H_raw[q] = 0.0;
        constraint_information(R.H_raw, R.H_prior, eigs);
    }
}

}  // namespace pinert
}  // namespace msorb
