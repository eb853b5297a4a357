// Optimizer::LocalInertialBA (src/Optimizer.cc:2431-2973) after its gathering loops, for pinhole KeyFrames without a second camera:
// the graph of EdgeMono / EdgeStereo (include/G2oTypes.h:342-388, :425-493, src/G2oTypes.cc:349-373, :397-427) over ImuCamPose and
// VertexSBAPointXYZ, EdgeInertial (G2oTypes.cc:492-594) and EdgeGyroRW / EdgeAccRW (G2oTypes.h:635-704) between consecutive
// KeyFrames, g2o's Levenberg (levenberg_device.h) with the user's lambda, the points eliminated by the Schur complement
// (core/block_solver.hpp:354-486), the classification of :2876-2904 and what the FAIL rule of :2911 reads.  One statement of the
// arithmetic for the device (local_inertial_ba.hip) and the host (tests/local_inertial_ba_main.cc): plain arithmetic in the order
// the reference writes it, a product of small matrices the row-by-column sum left to right, nothing contracted
// (-ffp-contract=off).  DESIGN.md section 24.
//
// The routine is a template over an executor: ex.tid(), ex.stride() (this executor's first item of a pass and the step to its next
// one; host: 0, 1) and ex.barrier() (everything written before it is visible to every executor after it).  Every pass hands out
// ITEMS (an edge, a point, an entry of the system, a row of a block) and an item's arithmetic does not depend on who computes it:
// every sum walks an index list of local_ba_plan.h, or a fixed run of slots, in ascending order.  So the device and the host
// program return the same bits, and two runs do.  All state lives in the Work block (global memory on the device).
//
// Unknowns in g2o's order (vertex ids among the free vertices): the free KeyFrames' poses, ascending, 6 each; then per free
// KeyFrame, ascending, velocity, gyro bias, acc bias, 9 each.  The system is dense, n = 15 Kf, kept as its LOWER triangle
// (row major, stride n).  The Schur complement touches the pose corner only.
//
// Order of the sums that the reference leaves to its containers:
//   entry (r, c) of H and entry r of b:  the visual edges' gather first (the KeyFrame's list, ascending edge), then the inertial
//       edges that touch both unknowns in ascending edge index, each as EdgeInertial, EdgeGyroRW, EdgeAccRW;
//   the cost: kSlots partial sums (slot q adds the visual edges q, q + kSlots, ... ascending), the slots ascending, then per
//       inertial edge ascending EdgeInertial's rho, EdgeGyroRW's chi2, EdgeAccRW's chi2;
//   computeScale: the same slots over the vertices (a free KeyFrame's fifteen terms ascending, a point's three).
//
// TWO states are kept apart at the end (see classify): the copy the last trial wrote (accepted or not), which the per-edge chi2
// in W.chi2 and err_end belong to because the reference reads chi2() without computeError(); and `cur`, the estimate.
#pragma once
#include "pose_inertial_device.h"

namespace msorb {
namespace liba {

using pinert::Cam;
using pinert::kJc;
using pinert::PoseEst;
using pinert::tri6;
using pinert::Vertices;
using eg4::dot3;
using eg4::mul33;
using eg4::mul3v;

constexpr int kCapacity = 25;      // free KeyFrames: the reference's maxOpt with bLarge (Optimizer.cc:2435-2440)
constexpr int kSlots = 256;
// planes of the edge-major linearisation, as ba_kernels_device.h
constexpr int kHll = 0, kBl = 6, kHpp = 9, kBp = 30, kW = 36, kPlanes = 54;

// one inertial edge's linearisation
struct IEdgeLin {
    double J[9 * kJc], AtO[kJc * 9], e[9], Oe[9];
    double rw[6];        // Omega e of EdgeGyroRW, EdgeAccRW
    double rho1;         // EdgeInertial's robust weight
    double cost[3];      // rho[0] of EdgeInertial, chi2 of EdgeGyroRW, of EdgeAccRW
};

struct Res { double chi, scale; };   // the cost and computeScale's sum, where every executor reads them after the barrier

struct Work {
    int K, Kf, P, E, NI, n, n_pairs, max_it, large;
    int shared_bias;                              // full_inertial_ba_device.h's init form: one bias pair for every edge, always free
    const msorb_iba_keyframe* kf;
    const msorb_iba_inertial_edge* ie;            // info already downweighted (staged_edge)
    const int *free_of_kf, *kf_of_free, *edge_kf, *edge_pt, *point_begin, *kf_begin, *kf_edge, *pair_begin, *pair_i, *pair_j, *pair_a, *pair_b;
    const int *e_in, *e_out;                      // [K]: the inertial edge that ends / starts at the KeyFrame, -1 = none
    const float *xy, *ur, *w;
    const uint8_t* close;
    Vertices* st[2];                              // the two copies of the KeyFrames' estimates (push / pop), [K] each
    double* pt[2];                                // of the points, [3 P] each
    double *lin, *Hpp, *Hll, *Dinv;               // [kPlanes][E], [Kf][27], [P][9], [P][9]
    double *A, *bA;                               // H without lambda [n][n] (lower), b [n]
    double *S, *bs, *x;                           // the reduced system of one trial, its right side, the solver's x
    double *col_v, *col_l, *y, *rd;               // [n] each: the solve's column, its scaled copy, the substitutions, 1 / D
    double *chi2, *rho0;                          // [E]: every visual edge's chi2() and rho[0] as last evaluated
    double *slots, *part_vtx;                     // [kSlots], [Kf + P]
    IEdgeLin* il;                                 // [NI]
    Res* res;
    uint8_t* outlier;                             // [E]
    msorb_iba_result* out;
};

// information() * 1e-2 (Optimizer.cc:2665), in double, entry by entry
inline msorb_iba_inertial_edge staged_edge(const msorb_iba_inertial_edge& in) {
    msorb_iba_inertial_edge e = in;
    if (e.downweight)
        for (int q = 0; q < 81; q++) e.pre.info[q] = e.pre.info[q] * 1e-2;
    return e;
}

SE3_HD void vertices_from(Vertices& V, const msorb_iba_keyframe& k) {
    for (int q = 0; q < 9; q++) { V.P.Rwb[q] = k.Rwb[q]; V.P.Rcw[q] = k.Rcw[q]; }   // ImuCamPose(pKF): Rcw / tcw from GetPose()
    for (int a = 0; a < 3; a++) { V.P.twb[a] = k.twb[a]; V.P.tcw[a] = k.tcw[a]; V.v[a] = k.v[a]; V.bg[a] = k.bg[a]; V.ba[a] = k.ba[a]; }
    V.P.its = 0;
}

// ---- the visual edges

struct VEdge { double e[3], Xc[3], chi2; bool stereo; };

// computeError (G2oTypes.h:353-358, :437-442 through ImuCamPose::Project / ProjectStereo, G2oTypes.cc:170-185) and chi2()
SE3_HD VEdge visual_error(const Work& W, int s, int e) {
    const int k = W.edge_kf[e];
    const PoseEst& T = W.st[s][k].P;
    const double* X = W.pt[s] + 3 * (size_t)W.edge_pt[e];
    const msorb_iba_keyframe& c = W.kf[k];
    VEdge g;
    double t[3];
    mul3v(T.Rcw, X, t);
    for (int a = 0; a < 3; a++) g.Xc[a] = t[a] + T.tcw[a];
    const double w = (double)W.w[e];
    const double p0 = ((double)c.fx * g.Xc[0]) / g.Xc[2] + (double)c.cx, p1 = ((double)c.fy * g.Xc[1]) / g.Xc[2] + (double)c.cy;
    g.e[0] = (double)W.xy[2 * (size_t)e] - p0;
    g.e[1] = (double)W.xy[2 * (size_t)e + 1] - p1;
    const float ur = W.ur[e];
    g.stereo = ur >= 0;
    if (g.stereo) {
        const double invZ = 1 / g.Xc[2];
        g.e[2] = (double)ur - (p0 - (double)c.mbf * invZ);
        g.chi2 = (g.e[0] * (w * g.e[0]) + g.e[1] * (w * g.e[1])) + g.e[2] * (w * g.e[2]);
    } else {
        g.e[2] = 0;
        g.chi2 = g.e[0] * (w * g.e[0]) + g.e[1] * (w * g.e[1]);
    }
    return g;
}

SE3_HD double huber_delta(bool stereo) { return stereo ? (double)(float)sqrt(7.815) : (double)(float)sqrt(5.991); }   // :2745-2746

// One visual edge of computeActiveErrors (+ buildSystem with FULL): its chi2 and rho[0] stored, and the terms of Hll / bl, Hpp / bp
// and W = Hpl (6x3) edge-major.  linearizeOplus is G2oTypes.cc:349-373, :397-427: the point's Jacobian -proj_jac Rcw, the pose's
// (proj_jac Rcb) SE3deriv(Xb); constructQuadraticForm is base_binary_edge.hpp:99-113.
template <bool FULL>
SE3_HD void visual_edge(const Work& W, int s, int e) {
    const VEdge g = visual_error(W, s, e);
    double rho0, rho1;
    se3::huber(g.chi2, huber_delta(g.stereo), true, rho0, rho1);
    W.chi2[e] = g.chi2;
    W.rho0[e] = rho0;
    if (!FULL) return;
    const int k = W.edge_kf[e];
    const msorb_iba_keyframe& c = W.kf[k];
    const PoseEst& T = W.st[s][k].P;
    const Cam cam{(double)c.fx, (double)c.fy, (double)c.cx, (double)c.cy, (double)c.mbf};
    const double zz = g.Xc[2] * g.Xc[2];
    double pj[9] = {cam.fx / g.Xc[2], 0.0, (-cam.fx * g.Xc[0]) / zz, 0.0, cam.fy / g.Xc[2], (-cam.fy * g.Xc[1]) / zz, 0.0, 0.0, 0.0};
    if (g.stereo) {
        const double inv_z2 = 1.0 / zz;
        pj[6] = pj[0]; pj[7] = pj[1]; pj[8] = pj[2] + cam.bf * inv_z2;
    }
    double Ja[3][3], Jb[3][6], M[9];
    mul33(pj, T.Rcw, M);
    for (int r = 0; r < 3; r++)
        for (int a = 0; a < 3; a++) Ja[r][a] = -M[3 * r + a];
    const size_t E = (size_t)W.E;
    double* L = W.lin + e;
    const int D = g.stereo ? 3 : 2;
    const double w = (double)W.w[e], wr = rho1 * w;
    double omr[3];
    for (int d = 0; d < 3; d++) omr[d] = (-(w * g.e[d])) * rho1;
    auto quad = [&](const double* ua, int sa, const double* ub, int sb) {
        double t = (ua[0] * wr) * ub[0] + (ua[sa] * wr) * ub[sb];
        if (D == 3) t += (ua[2 * sa] * wr) * ub[2 * sb];
        return t;
    };
    auto dotr = [&](const double* ua, int sa) {
        double t = ua[0] * omr[0] + ua[sa] * omr[1];
        if (D == 3) t += ua[2 * sa] * omr[2];
        return t;
    };
    int q = kHll;
    for (int a = 0; a < 3; a++)
        for (int b = a; b < 3; b++) L[(size_t)(q++) * E] = quad(&Ja[0][a], 3, &Ja[0][b], 3);
    for (int a = 0; a < 3; a++) L[(size_t)(kBl + a) * E] = dotr(&Ja[0][a], 3);
    if (W.free_of_kf[k] < 0) return;   // a fixed vertex has no column
    pinert::visual_jacobian(cam, g.stereo, g.Xc, c.Rcb, c.tbc, Jb);
    q = kHpp;
    for (int a = 0; a < 6; a++)
        for (int b = a; b < 6; b++) L[(size_t)(q++) * E] = quad(&Jb[0][a], 6, &Jb[0][b], 6);
    for (int a = 0; a < 6; a++) L[(size_t)(kBp + a) * E] = dotr(&Jb[0][a], 6);
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 3; b++) L[(size_t)(kW + 3 * a + b) * E] = quad(&Jb[0][a], 6, &Ja[0][b], 3);
}

// ---- the inertial edges

SE3_HD bool iedge_active(const Work& W, int i) {   // an edge whose vertices are all fixed is not active
    return W.shared_bias || W.free_of_kf[W.ie[i].pre.kf_prev] >= 0 || W.free_of_kf[W.ie[i].pre.kf_cur] >= 0;
}

// EdgeInertial, EdgeGyroRW and EdgeAccRW number i at state s: errors, chi2, EdgeInertial's Huber of delta sqrt(16.92)
// (Optimizer.cc:2657-2667) and, with jac, the Jacobian.  1 = kf_prev, 2 = kf_cur.
INERTIAL_OUT_OF_LINE SE3_HD void inertial_edge(const Work& W, int s, int i, bool jac) {
    const msorb_iba_inertial_edge& E = W.ie[i];
    IEdgeLin& L = W.il[i];
    if (!iedge_active(W, i)) { L.cost[0] = L.cost[1] = L.cost[2] = 0; return; }
    const Vertices& O = W.st[s][E.pre.kf_prev];
    const Vertices& F = W.st[s][E.pre.kf_cur];
    if (jac)
        for (int q = 0; q < 9 * kJc; q++) L.J[q] = 0.0;
    pinert::inertial_edge_terms(E.pre, E.pre.info, F, O, jac, L.J, L.e, L.Oe);
    double chi = L.e[0] * L.Oe[0];
    for (int r = 1; r < 9; r++) chi += L.e[r] * L.Oe[r];
    double rho0;
    se3::huber(chi, sqrt(16.92), E.huber != 0, rho0, L.rho1);
    L.cost[0] = rho0;
    double eg[3], ea[3], t[3];
    for (int a = 0; a < 3; a++) { eg[a] = F.bg[a] - O.bg[a]; ea[a] = F.ba[a] - O.ba[a]; }   // G2oTypes.h:645-649, :681-685
    mul3v(E.info_gyro, eg, t);
    for (int a = 0; a < 3; a++) L.rw[a] = t[a];
    L.cost[1] = (eg[0] * t[0] + eg[1] * t[1]) + eg[2] * t[2];
    mul3v(E.info_acc, ea, t);
    for (int a = 0; a < 3; a++) L.rw[3 + a] = t[a];
    L.cost[2] = (ea[0] * t[0] + ea[1] * t[1]) + ea[2] * t[2];
}

// unknown r -> its free KeyFrame and its place among that KeyFrame's fifteen (pose 0-5, velocity 6-8, gyro bias 9-11, acc 12-14)
SE3_HD void unknown_of(const Work& W, int r, int& i, int& u) {
    if (r < 6 * W.Kf) { i = r / 6; u = r % 6; }
    else { i = (r - 6 * W.Kf) / 9; u = 6 + (r - 6 * W.Kf) % 9; }
}
SE3_HD int unknown_at(const Work& W, int i, int u) { return u < 6 ? 6 * i + u : 6 * W.Kf + 9 * i + (u - 6); }

// EdgeInertial's column of place u of KeyFrame k (-1: none): kf_prev's fifteen are its columns 0..14, kf_cur's pose and velocity
// its columns 15..23
SE3_HD int iedge_col(const msorb_iba_inertial_edge& E, int k, int u) { return k == E.pre.kf_prev ? u : (u < 9 ? 15 + u : -1); }

// what inertial edge m adds to entry (r, c) of H: places (ka, ua), (kb, ub)
SE3_HD double iedge_entry(const Work& W, int m, int ka, int ua, int kb, int ub) {
    const msorb_iba_inertial_edge& E = W.ie[m];
    const IEdgeLin& L = W.il[m];
    double v = 0;
    const int a = iedge_col(E, ka, ua), b = iedge_col(E, kb, ub);
    if (a >= 0 && b >= 0) {
        double t = L.AtO[a * 9] * L.J[b];
        for (int q = 1; q < 9; q++) t += L.AtO[a * 9 + q] * L.J[q * kJc + b];
        v = t;
    }
    // J = [-I | I] on (prev, cur): omega on both diagonal blocks, -omega between them (G2oTypes.h:651-662)
    const bool same = ka == kb;
    if (ua >= 9 && ua < 12 && ub >= 9 && ub < 12) v += same ? E.info_gyro[3 * (ua - 9) + (ub - 9)] : -E.info_gyro[3 * (ua - 9) + (ub - 9)];
    if (ua >= 12 && ub >= 12) v += same ? E.info_acc[3 * (ua - 12) + (ub - 12)] : -E.info_acc[3 * (ua - 12) + (ub - 12)];
    return v;
}

// what inertial edge m adds to entry r of b: A^T (-(rho' omega e)), then the random walks'
SE3_HD double iedge_b(const Work& W, int m, int k, int u) {
    const msorb_iba_inertial_edge& E = W.ie[m];
    const IEdgeLin& L = W.il[m];
    double v = 0;
    const int a = iedge_col(E, k, u);
    if (a >= 0) {
        double t = L.J[a] * -(L.rho1 * L.Oe[0]);
        for (int q = 1; q < 9; q++) t += L.J[q * kJc + a] * -(L.rho1 * L.Oe[q]);
        v = t;
    }
    if (u >= 9) v += k == E.pre.kf_cur ? -L.rw[u - 9] : L.rw[u - 9];   // cur: I^T (-(omega e)); prev: (-I)^T (-(omega e))
    return v;
}

// ---- sums in a fixed order

// sum of v[0, n) into *out: slot q adds q, q + kSlots, ...; executor 0 adds the slots ascending, then extra[0, n_extra)
template <typename Exec>
SE3_HD void slot_sum(Exec& ex, const Work& W, const double* v, int n, const double* extra, int n_extra, int extra_stride, int extra_each,
                     double* out) {
    for (int q = ex.tid(); q < kSlots; q += ex.stride()) {
        double s = 0;
        for (int i = q; i < n; i += kSlots) s += v[i];
        W.slots[q] = s;
    }
    ex.barrier();
    if (ex.tid() == 0) {
        double s = W.slots[0];
        for (int q = 1; q < kSlots; q++) s += W.slots[q];
        for (int i = 0; i < n_extra; i++)
            for (int j = 0; j < extra_each; j++) s += extra[(size_t)i * extra_stride + j];
        *out = s;
    }
    ex.barrier();
}

// activeRobustChi2 over the errors as last evaluated
template <typename Exec>
SE3_HD double cost(Exec& ex, const Work& W) {
    slot_sum(ex, W, W.rho0, W.E, W.NI ? W.il[0].cost : nullptr, W.NI, (int)(sizeof(IEdgeLin) / sizeof(double)), 3, &W.res->chi);
    return W.res->chi;
}

// ---- the passes

// computeActiveErrors (+ buildSystem) at state s
template <bool FULL, typename Exec>
SE3_HD void evaluate(Exec& ex, const Work& W, int s) {
    for (int e = ex.tid(); e < W.E; e += ex.stride()) visual_edge<FULL>(W, s, e);
    for (int i = ex.tid(); i < W.NI; i += ex.stride()) inertial_edge(W, s, i, FULL);
    ex.barrier();
}

// Hll / bl of point p over its run of edges, ascending
SE3_HD void point_gather(const Work& W, int p) {
    const size_t E = (size_t)W.E;
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int e = W.point_begin[p]; e < W.point_begin[p + 1]; e++)
        for (int q = 0; q < 9; q++) S[q] += W.lin[(size_t)q * E + e];
    for (int q = 0; q < 9; q++) W.Hll[9 * (size_t)p + q] = S[q];
}

// entry t % 27 of Hpp / bp of free KeyFrame t / 27 over its list, ascending
SE3_HD void hpp_gather(const Work& W, int t) {
    const size_t E = (size_t)W.E;
    const int i = t / 27, q = t % 27;
    double s = 0;
    for (int m = W.kf_begin[i]; m < W.kf_begin[i + 1]; m++) s += W.lin[(size_t)(kHpp + q) * E + W.kf_edge[m]];
    W.Hpp[t] = s;
}

// entry t % (kJc * 9) of inertial edge t / (kJc * 9)'s A^T (rho' omega): robustInformation (base_edge.h:96-100)
SE3_HD void ato_entry(const Work& W, int t, bool active) {
    const int m = t / (kJc * 9), q = t % (kJc * 9), a = q / 9, c = q % 9;
    if (!active) return;
    IEdgeLin& L = W.il[m];
    const double* info = W.ie[m].pre.info;
    double s = L.J[a] * (L.rho1 * info[c]);
    for (int k = 1; k < 9; k++) s += L.J[k * kJc + a] * (L.rho1 * info[9 * k + c]);
    L.AtO[q] = s;
}

// Hll / bl per point, Hpp / bp per free KeyFrame over its list, the inertial edges' A^T (rho' omega), then H and b
template <typename Exec>
SE3_HD void build_system(Exec& ex, const Work& W) {
    const int n = W.n;
    for (int p = ex.tid(); p < W.P; p += ex.stride()) point_gather(W, p);
    for (int t = ex.tid(); t < 27 * W.Kf; t += ex.stride()) hpp_gather(W, t);
    for (int t = ex.tid(); t < W.NI * kJc * 9; t += ex.stride()) ato_entry(W, t, iedge_active(W, t / (kJc * 9)));
    ex.barrier();
    for (int t = ex.tid(); t < n * (n + 1); t += ex.stride()) {
        const int r = t / (n + 1), c = t % (n + 1);
        if (c < n && c > r) continue;
        int ia, ua, ib = 0, ub = 0;
        unknown_of(W, r, ia, ua);
        const int ka = W.kf_of_free[ia];
        if (c == n) {
            double v = ua < 6 ? W.Hpp[27 * (size_t)ia + 21 + ua] : 0.0;
            // the edge that ends here comes before the one that starts here exactly when its index is lower
            const int m0 = W.e_in[ka], m1 = W.e_out[ka];
            const int lo = m0 >= 0 && (m1 < 0 || m0 < m1) ? m0 : m1, hi = lo == m0 ? m1 : m0;
            if (lo >= 0) v += iedge_b(W, lo, ka, ua);
            if (hi >= 0 && hi != lo) v += iedge_b(W, hi, ka, ua);
            W.bA[r] = v;
            continue;
        }
        unknown_of(W, c, ib, ub);
        const int kb = W.kf_of_free[ib];
        double v = (ia == ib && ua < 6 && ub < 6) ? W.Hpp[27 * (size_t)ia + (ua <= ub ? tri6(ua, ub) : tri6(ub, ua))] : 0.0;
        const int ma[2] = {W.e_in[ka], W.e_out[ka]};
        int hit[2] = {-1, -1};
        for (int j = 0; j < 2; j++)
            if (ma[j] >= 0 && (ma[j] == W.e_in[kb] || ma[j] == W.e_out[kb])) hit[j] = ma[j];
        if (hit[0] >= 0 && hit[1] >= 0 && hit[1] < hit[0]) { const int z = hit[0]; hit[0] = hit[1]; hit[1] = z; }
        // (c, r) is the upper-triangle entry the reference forms: the lower one holds its value
        for (int j = 0; j < 2; j++)
            if (hit[j] >= 0) v += iedge_entry(W, hit[j], kb, ub, ka, ua);
        W.A[(size_t)r * n + c] = v;
    }
    ex.barrier();
}

// Dinv of point p (block_solver.hpp:389) as Eigen inverts a 3x3, with setLambda on Hll (:573-578), and Dinv bl
SE3_HD void dinv_point(const Work& W, int p, double lambda) {
    const double* H = W.Hll + 9 * (size_t)p;
    const double m00 = H[0] + lambda, m01 = H[1], m02 = H[2], m11 = H[3] + lambda, m12 = H[4], m22 = H[5] + lambda;
    const double c00 = m11 * m22 - m12 * m12, c10 = m12 * m02 - m22 * m01, c20 = m01 * m12 - m02 * m11;
    const double det = (c00 * m00 + c10 * m01) + c20 * m02, inv = 1.0 / det;
    const double i00 = c00 * inv, i01 = c10 * inv, i02 = c20 * inv;
    const double i11 = (m22 * m00 - m02 * m02) * inv, i12 = (m02 * m01 - m00 * m12) * inv, i22 = (m00 * m11 - m01 * m01) * inv;
    double* o = W.Dinv + 9 * (size_t)p;
    o[0] = i00; o[1] = i01; o[2] = i02; o[3] = i11; o[4] = i12; o[5] = i22;
    o[6] = (i00 * H[6] + i01 * H[7]) + i02 * H[8];
    o[7] = (i01 * H[6] + i11 * H[7]) + i12 * H[8];
    o[8] = (i02 * H[6] + i12 * H[7]) + i22 * H[8];
}

// One task of the Schur complement (:381-439): row t % 6 of block pair t / 6 (i <= j) taken off S, or row t % 6 of a KeyFrame's
// right side.  S and bs hold the system with lambda set; the pose corner is rows and columns 0 .. 6 Kf of the stride-n square.
SE3_HD void schur_task(const Work& W, int t) {
    const size_t E = (size_t)W.E;
    const int n = W.n;
    const int task = t / 6, r = t % 6;
    if (task >= W.n_pairs) {
        const int i = task - W.n_pairs;
        double c = 0;
        for (int m = W.kf_begin[i]; m < W.kf_begin[i + 1]; m++) {
            const int e = W.kf_edge[m];
            const double* db = W.Dinv + 9 * (size_t)W.edge_pt[e] + 6;
            const double* Wr = W.lin + (size_t)(kW + 3 * r) * E + e;
            c += (Wr[0] * db[0] + Wr[E] * db[1]) + Wr[2 * E] * db[2];
        }
        W.bs[6 * i + r] = W.bA[6 * i + r] - c;
        return;
    }
    const int i = W.pair_i[task], j = W.pair_j[task];
    double T[6] = {0, 0, 0, 0, 0, 0};
    for (int m = W.pair_begin[task]; m < W.pair_begin[task + 1]; m++) {
        const int a = W.pair_a[m], b = W.pair_b[m];
        const double* Di = W.Dinv + 9 * (size_t)W.edge_pt[a];
        const double w0 = W.lin[(size_t)(kW + 3 * r) * E + a], w1 = W.lin[(size_t)(kW + 3 * r + 1) * E + a],
                     w2 = W.lin[(size_t)(kW + 3 * r + 2) * E + a];
        const double y0 = (w0 * Di[0] + w1 * Di[1]) + w2 * Di[2], y1 = (w0 * Di[1] + w1 * Di[3]) + w2 * Di[4],
                     y2 = (w0 * Di[2] + w1 * Di[4]) + w2 * Di[5];
        for (int c = 0; c < 6; c++)
            T[c] += (y0 * W.lin[(size_t)(kW + 3 * c) * E + b] + y1 * W.lin[(size_t)(kW + 3 * c + 1) * E + b]) +
                    y2 * W.lin[(size_t)(kW + 3 * c + 2) * E + b];
    }
    for (int c = (i == j ? r : 0); c < 6; c++) {
        double* s = W.S + (size_t)(6 * j + c) * n + 6 * i + r;
        *s = *s - T[c];
    }
}

// setLambda on all of Hpp and Hll (block_solver.hpp:573-578), Dinv (:389) as Eigen inverts a 3x3, the Schur complement over the
// plan's lists (:381-439) into the pose corner
template <typename Exec>
SE3_HD void reduce_system(Exec& ex, const Work& W, double lambda) {
    const int n = W.n;
    for (int p = ex.tid(); p < W.P; p += ex.stride()) dinv_point(W, p, lambda);
    for (int t = ex.tid(); t < n * n; t += ex.stride()) {
        const int r = t / n, c = t % n;
        if (c <= r) W.S[t] = r == c ? W.A[t] + lambda : W.A[t];
    }
    for (int r = ex.tid(); r < n; r += ex.stride()) W.bs[r] = W.bA[r];
    ex.barrier();
    // a task = one row of one block pair (i <= j), or one row of a KeyFrame's right side
    const int n_tasks = 6 * (W.n_pairs + W.Kf);
    for (int t = ex.tid(); t < n_tasks; t += ex.stride()) schur_task(W, t);
    ex.barrier();
}

// S = L D L^T without pivoting and without a square root, right-looking over the lower triangle, then the two substitutions:
// ba_solve_kernel's arithmetic (bundle_adjustment.hip), column m's update of entry (i, k) is - L[i][m] (L[k][m] D[m]) for m
// ascending.  A pivot that is not > 0: false, x keeps what it held.  Every executor takes the same path.
template <typename Exec>
SE3_HD bool solve(Exec& ex, const Work& W) {
    const int n = W.n;
    double* S = W.S;
    for (int j = 0; j < n; j++) {
        const double d = S[(size_t)j * n + j];
        if (!(d > 0)) { ex.barrier(); return false; }
        const double r = 1.0 / d;
        if (ex.tid() == 0) W.rd[j] = r;
        for (int i = j + 1 + ex.tid(); i < n; i += ex.stride()) {
            const double s = S[(size_t)i * n + j];
            W.col_v[i] = s;
            W.col_l[i] = s * r;
            S[(size_t)i * n + j] = s * r;
        }
        ex.barrier();
        // the trailing lower triangle, m rows of 1 .. m entries: row a and row m - 1 - a together are m + 1 items, so
        // ceil(m / 2) stripes of m + 1 hold every entry once (the middle row of an odd m is a stripe's first half alone)
        const int m = n - 1 - j, stripes = (m + 1) / 2;
        for (int q = ex.tid(); q < stripes * (m + 1); q += ex.stride()) {
            const int a = q / (m + 1), b = q % (m + 1);
            if (b > a && m - 1 - a == a) continue;
            const int r = b <= a ? a : m - 1 - a, c = b <= a ? b : b - a - 1;
            const int i = j + 1 + r, k = j + 1 + c;
            S[(size_t)i * n + k] -= W.col_l[i] * W.col_v[k];
        }
        ex.barrier();
    }
    for (int i = ex.tid(); i < n; i += ex.stride()) W.y[i] = W.bs[i];
    ex.barrier();
    for (int m = 0; m < n; m++) {
        const double ym = W.y[m];
        ex.barrier();
        for (int i = m + 1 + ex.tid(); i < n; i += ex.stride()) W.y[i] -= S[(size_t)i * n + m] * ym;
        ex.barrier();
    }
    for (int i = ex.tid(); i < n; i += ex.stride()) W.y[i] *= W.rd[i];
    ex.barrier();
    for (int m = n - 1; m >= 0; m--) {
        const double xm = W.y[m];
        ex.barrier();
        for (int i = ex.tid(); i < m; i += ex.stride()) W.y[i] -= S[(size_t)m * n + i] * xm;
        ex.barrier();
    }
    for (int i = ex.tid(); i < n; i += ex.stride()) W.x[i] = W.y[i];
    ex.barrier();
    return true;
}

// xl = Dinv (bl - sum W^T xp) of point p (block_solver.hpp:461-481) added to copy `from` into copy `to`, and the point's term of
// computeScale (levenberg.cpp:188-195) into part_vtx[slot]
SE3_HD void point_update(const Work& W, int from, int to, double lambda, int p, int slot) {
    const size_t E = (size_t)W.E;
    const double* H = W.Hll + 9 * (size_t)p;
    double cl[3] = {H[6], H[7], H[8]};
    for (int e = W.point_begin[p]; e < W.point_begin[p + 1]; e++) {
        const int i = W.free_of_kf[W.edge_kf[e]];
        if (i < 0) continue;
        const double* xp = W.x + 6 * (size_t)i;
        for (int c = 0; c < 3; c++) {
            double tsum = 0;
            for (int r = 0; r < 6; r++) tsum += W.lin[(size_t)(kW + 3 * r + c) * E + e] * (-xp[r]);
            cl[c] += tsum;
        }
    }
    const double* D = W.Dinv + 9 * (size_t)p;
    double xl[3];
    xl[0] = (D[0] * cl[0] + D[1] * cl[1]) + D[2] * cl[2];
    xl[1] = (D[1] * cl[0] + D[3] * cl[1]) + D[4] * cl[2];
    xl[2] = (D[2] * cl[0] + D[4] * cl[1]) + D[5] * cl[2];
    double sc = 0;
    for (int c = 0; c < 3; c++) {
        sc += xl[c] * (lambda * xl[c] + H[6 + c]);
        W.pt[to][3 * (size_t)p + c] = W.pt[from][3 * (size_t)p + c] + xl[c];
    }
    W.part_vtx[slot] = sc;
}

// SparseOptimizer::update of copy `from` into copy `to` (sparse_optimizer.cpp:422-441): a free KeyFrame's four oplusImpl (the copy
// carries ImuCamPose's update counter, so push / pop keep it as the reference's copy of the estimate does), and per point
// xl = Dinv (bl - sum W^T xp) (block_solver.hpp:461-481); computeScale's terms (levenberg.cpp:188-195) per vertex
template <typename Exec>
SE3_HD void update(Exec& ex, const Work& W, int from, int to, double lambda) {
    for (int v = ex.tid(); v < W.Kf + W.P; v += ex.stride()) {
        if (v < W.Kf) {
            const int k = W.kf_of_free[v];
            double u[15], sc = 0;
            for (int a = 0; a < 15; a++) {
                const int r = unknown_at(W, v, a);
                u[a] = W.x[r];
                sc += u[a] * (lambda * u[a] + W.bA[r]);
            }
            Vertices V = W.st[from][k];
            pinert::vertices_update(V, u, W.kf[k].Rcb, W.kf[k].tcb);
            W.st[to][k] = V;
            W.part_vtx[v] = sc;
            continue;
        }
        point_update(W, from, to, lambda, v - W.Kf, v);
    }
    ex.barrier();
}

// The classification of Optimizer.cc:2876-2904.  It calls chi2() WITHOUT computeError(): W.chi2 holds every edge's chi2 at the
// state the last trial wrote, accepted or not (levenberg.cpp:123, then pop() at :146), while isDepthPositive() reads the
// estimate, copy `cur`.  The thresholds are floats (5.991f, 1.5f * 5.991f for a close point, 7.815f) against the double chi2.
SE3_HD uint8_t classify(const Work& W, int cur, int e) {
    const double c = W.chi2[e];
    if (W.ur[e] >= 0) return c > (double)7.815f ? 1 : 0;
    const int p = W.edge_pt[e];
    const PoseEst& T = W.st[cur][W.edge_kf[e]].P;
    const double* X = W.pt[cur] + 3 * (size_t)p;
    const bool close = W.close[p] != 0;
    const bool depth_ok = dot3(T.Rcw[6], T.Rcw[7], T.Rcw[8], X[0], X[1], X[2]) + T.tcw[2] > 0.0;
    return ((c > (double)5.991f && !close) || (c > (double)(1.5f * 5.991f) && close) || !depth_ok) ? 1 : 0;
}

// One call.  Copy 0 of the state holds the inputs; x is zero.  Returns the copy that holds the estimate; executor 0 writes *W.out
// (status 0 or 1; the caller decides what a status 1 hands back).
template <typename Exec>
SE3_HD int optimize(Exec& ex, const Work& W) {
    int cur = 0;
    double chi2_end = 0;
    bool evaluated = false;
    const lm::Counts n = lm::levenberg(
        W.max_it, true, W.large ? 1e-2 : 1e0,                                  // setUserLambdaInit (Optimizer.cc:2547-2555)
        [&](double& max_diagonal) {
            max_diagonal = 0;                                                  // (computeLambdaInit takes the user's value)
            evaluate<true>(ex, W, cur);
            build_system(ex, W);
            evaluated = true;
            return chi2_end = cost(ex, W);
        },
        [&](double lambda, bool& solved, double& scale) {
            reduce_system(ex, W, lambda);
            solved = solve(ex, W);
            update(ex, W, cur, cur ^ 1, lambda);                               // also when the solve failed: with the x it held
            evaluate<false>(ex, W, cur ^ 1);                                   // W.chi2 now belongs to the trial's copy
            slot_sum(ex, W, W.part_vtx, W.Kf + W.P, nullptr, 0, 0, 0, &W.res->scale);
            scale = W.res->scale;
            return chi2_end = cost(ex, W);
        },
        [&] { cur ^= 1; });
    double chi2_initial = n.chi2_initial;
    if (!evaluated) {                                                          // no iteration: Optimizer.cc:2864-2865 alone
        evaluate<false>(ex, W, cur);
        chi2_initial = chi2_end = cost(ex, W);
    }
    // W.chi2 is the chi2 at the copy the last evaluation read (the last trial's, accepted or not); the depth test reads copy `cur`
    for (int e = ex.tid(); e < W.E; e += ex.stride()) W.outlier[e] = classify(W, cur, e);
    ex.barrier();
    if (ex.tid() == 0) {
        msorb_iba_result& R = *W.out;
        const float err = (float)chi2_initial, err_end = (float)chi2_end;      // Optimizer.cc:2865-2867
        R.status = ((2 * err < err_end || err != err || err_end != err_end) && !W.large) ? 1 : 0;   // :2911
        R.iterations = n.iterations;
        R.trials = n.trials;
        R.rejected_trials = n.rejected;
        R.n_outliers = 0;
        R.reserved = 0;
        R.chi2_initial = chi2_initial;
        R.chi2_final = chi2_end;
        R.lambda_final = n.lambda;
        R.err = err;
        R.err_end = err_end;
    }
    ex.barrier();
    return cur;
}

// what the caller's setters receive (Optimizer.cc:2936-2948), next to the doubles
inline void keyframe_out(const Vertices& V, msorb_iba_keyframe_out& o) {
    for (int q = 0; q < 9; q++) { o.Rwb[q] = V.P.Rwb[q]; o.Rcw[q] = V.P.Rcw[q]; o.Rcw_f[q] = (float)V.P.Rcw[q]; }   // :2937
    for (int a = 0; a < 3; a++) {
        o.twb[a] = V.P.twb[a]; o.tcw[a] = V.P.tcw[a]; o.v[a] = V.v[a]; o.bg[a] = V.bg[a]; o.ba[a] = V.ba[a];
        o.tcw_f[a] = (float)V.P.tcw[a];
        o.v_f[a] = (float)V.v[a];             // :2943
        o.bias_f[a] = (float)V.ba[a];         // :2946-2948: IMU::Bias(b[3], b[4], b[5], b[0], b[1], b[2]) = acc, then gyro
        o.bias_f[3 + a] = (float)V.bg[a];
    }
    o.reserved_f = 0;
}

// the FAIL rule alone, for callers that test it with hand-set values
inline bool fail_rule(float err, float err_end, bool large) { return (2 * err < err_end || std::isnan(err) || std::isnan(err_end)) && !large; }

}  // namespace liba
}  // namespace msorb
