// Optimizer::FullInertialBA (src/Optimizer.cc:366-756) after its gathering loops, for pinhole KeyFrames without a second camera:
// g2o's optimize(its) over the whole inertial map.  The edges, their sums and the Schur rows are the ITEM functions of
// local_inertial_ba_device.h (visual_edge, inertial_edge, iedge_entry, iedge_b, point_gather, hpp_gather, ato_entry, dinv_point,
// schur_task, point_update, vertices_update); this header states what FullInertialBA does differently and cuts the routine into
// PASSES without a barrier inside, so that the host can drive them launch by launch over the whole chip and look at the stop
// flag where g2o calls terminate().  The same text is read by hipcc (full_inertial_ba.hip) and by g++
// (tests/full_inertial_ba_main.cc), with -ffp-contract=off.  DESIGN.md section 25.
//
// Two graphs (bInit):
//   init = 0   per free KeyFrame pose, velocity, gyro bias, acc bias; EdgeInertial with Huber sqrt(16.92) and its information as
//              given, EdgeGyroRW, EdgeAccRW (:491-522).  Unknowns as section 24: the poses, 6 each, then 9 per KeyFrame; n = 15 Kf.
//              An inertial edge between two fixed KeyFrames is not active (sparse_optimizer.cpp:227-234).
//   init = 1   per free KeyFrame pose and velocity; ONE gyro bias and one acc bias, always free, shared by every EdgeInertial
//              (:427-436, ids 4 maxKFid + 2 / + 3: the last of the non-marginalised unknowns); no random-walk edge; EdgePriorAcc
//              and EdgePriorGyro with bprior = 0 (:528-547).  Unknowns: the poses, then 3 per KeyFrame, then gyro 3, acc 3;
//              n = 9 Kf + 6.  Every inertial edge is active, because the shared biases are free.
//              Every KeyFrame's copy of the state carries the shared pair in its bg / ba, every update moves all of them by the
//              same six numbers, and the random-walk informations are staged as zero: so inertial_edge, iedge_entry and iedge_b
//              read what they read in the other form (the bias columns of EdgeInertial are those of its kf_prev).
//
// Order of the sums the reference leaves to its containers, beyond section 24's:
//   an entry of H or b on a KeyFrame's unknowns: the visual gather, then the (at most two) inertial edges at the KeyFrame ascending;
//   an entry on the shared biases alone: every inertial edge ascending, then the prior;
//   the cost: the visual edges' 256 slots, the inertial edges ascending, then EdgePriorAcc, EdgePriorGyro;
//   computeScale: 256 slots over [free KeyFrames | points | the shared pair].
//
// The reduced system: the square is cleared once per trial, then `prepare` writes the entries that can be non-zero (a KeyFrame's
// own block, the block between two free KeyFrames of one inertial edge, the border and corner of the shared pair) with lambda on
// the diagonal, and `schur` takes the plan's block pairs off the pose corner.
#pragma once
#include <string>
#include <vector>

#include "local_ba_plan.h"
#include "local_inertial_ba_device.h"

namespace msorb {
namespace fiba {

using liba::kJc;
using liba::kSlots;
using pinert::tri6;
using pinert::Vertices;

constexpr int kMaxN = 7168;        // the side of the dense square ldlt_blocked.h is given (411 MB)
inline int capacity(int init) { return init ? (kMaxN - 6) / 9 : kMaxN / 15; }   // free KeyFrames: 795, 477

struct Res { double chi, scale; int solver_ok, pad; };

struct Work {
    liba::Work L;                  // L.n = n; L.part_vtx [Kf + P + 1]; L.A is not used: H is written into S per trial
    int init, per, nb;             // per: unknowns of a free KeyFrame after its pose (9 / 3); nb: the first shared unknown
    int n_fp;                      // inertial edges with both KeyFrames free
    int bias_kf;                   // a KeyFrame whose copy of the shared pair the priors read
    const int* fp_edge;            // [n_fp], ascending
    // A free KeyFrame without inertial vertices (kind 3, merge_inertial_ba_device.h) has its six pose unknowns alone.  inert_of_free
    // [Kf]: a free KeyFrame's index among those that have the `per` further unknowns, or -1; free_of_inert [Ki]: back.  Both null:
    // every free KeyFrame has them (FullInertialBA).
    const int *inert_of_free, *free_of_inert;
    double prior_g, prior_a;
    Res* res;
};

SE3_HD int places(const Work& F) { return 6 + F.per; }                     // of a free KeyFrame that has inertial vertices
SE3_HD int inert_of(const Work& F, int i) { return F.inert_of_free ? F.inert_of_free[i] : i; }
SE3_HD int places(const Work& F, int i) { return inert_of(F, i) >= 0 ? 6 + F.per : 6; }
SE3_HD int unknown_at(const Work& F, int i, int u) { return u < 6 ? 6 * i + u : 6 * F.L.Kf + F.per * inert_of(F, i) + (u - 6); }
SE3_HD void unknown_of(const Work& F, int r, int& i, int& u) {
    const int np = 6 * F.L.Kf;
    if (r < np) { i = r / 6; u = r % 6; }
    else {
        const int j = (r - np) / F.per;
        i = F.free_of_inert ? F.free_of_inert[j] : j;
        u = 6 + (r - np) % F.per;
    }
}

// the inertial edges at KeyFrame k, ascending: the one that ends there comes before the one that starts there exactly when its
// index is lower
SE3_HD void edges_at(const liba::Work& W, int k, int& lo, int& hi) {
    const int m0 = W.e_in[k], m1 = W.e_out[k];
    lo = m0 >= 0 && (m1 < 0 || m0 < m1) ? m0 : m1;
    hi = lo == m0 ? m1 : m0;
    if (hi == lo) hi = -1;
}

// ---- entries of H (without lambda) and b.  (c, r) is the upper-triangle entry the reference forms; the lower one holds its value.

// both unknowns on free KeyFrame i: places ur (row) >= uc (column) in the order of the unknowns
SE3_HD double entry_self(const Work& F, int i, int ur, int uc) {
    const liba::Work& W = F.L;
    const int k = W.kf_of_free[i];
    double v = (ur < 6 && uc < 6) ? W.Hpp[27 * (size_t)i + (ur <= uc ? tri6(ur, uc) : tri6(uc, ur))] : 0.0;
    int lo, hi;
    edges_at(W, k, lo, hi);
    if (lo >= 0) v += liba::iedge_entry(W, lo, k, uc, k, ur);
    if (hi >= 0) v += liba::iedge_entry(W, hi, k, uc, k, ur);
    return v;
}

// the unknowns of a shared bias (j = 0..5: gyro, acc) against place u of free KeyFrame i
SE3_HD double entry_border(const Work& F, int i, int u, int j) {
    const liba::Work& W = F.L;
    const int k = W.kf_of_free[i];
    double v = 0.0;
    int lo, hi;
    edges_at(W, k, lo, hi);
    if (lo >= 0) v += liba::iedge_entry(W, lo, k, u, W.ie[lo].pre.kf_prev, 9 + j);
    if (hi >= 0) v += liba::iedge_entry(W, hi, k, u, W.ie[hi].pre.kf_prev, 9 + j);
    return v;
}

// shared bias jr (row) against jc (column), jc <= jr: every inertial edge ascending, then the prior (information p I)
SE3_HD double entry_corner(const Work& F, int jr, int jc) {
    const liba::Work& W = F.L;
    double v = 0.0;
    for (int m = 0; m < W.NI; m++) v += liba::iedge_entry(W, m, W.ie[m].pre.kf_prev, 9 + jc, W.ie[m].pre.kf_prev, 9 + jr);
    if (jr == jc) v += jr < 3 ? F.prior_g : F.prior_a;
    return v;
}

// entry r of b at copy s (the priors read the shared pair there): linearizeOplus of both priors is the identity
// (G2oTypes.cc:762-775), error = bprior - estimate with bprior = 0, so b += -(p (0 - bias))
SE3_HD double entry_b(const Work& F, int s, int r) {
    const liba::Work& W = F.L;
    if (F.init && r >= F.nb) {
        const int j = r - F.nb;
        double v = 0.0;
        for (int m = 0; m < W.NI; m++) v += liba::iedge_b(W, m, W.ie[m].pre.kf_prev, 9 + j);
        const Vertices& B = W.st[s][F.bias_kf];
        v += j < 3 ? -(F.prior_g * (0.0 - B.bg[j])) : -(F.prior_a * (0.0 - B.ba[j - 3]));
        return v;
    }
    int i, u;
    unknown_of(F, r, i, u);
    const int k = W.kf_of_free[i];
    double v = u < 6 ? W.Hpp[27 * (size_t)i + 21 + u] : 0.0;
    int lo, hi;
    edges_at(W, k, lo, hi);
    if (lo >= 0) v += liba::iedge_b(W, lo, k, u);
    if (hi >= 0) v += liba::iedge_b(W, hi, k, u);
    return v;
}

// ---- the passes: loops over items, no barrier inside; each needs everything the passes before it wrote

// computeActiveErrors (+ the edges' part of buildSystem with FULL) at copy s
template <bool FULL, typename Exec>
SE3_HD void pass_edges(Exec& ex, const Work& F, int s) {
    const liba::Work& W = F.L;
    for (int e = ex.tid(); e < W.E; e += ex.stride()) liba::visual_edge<FULL>(W, s, e);
    for (int i = ex.tid(); i < W.NI; i += ex.stride()) liba::inertial_edge(W, s, i, FULL);
}

// Hll / bl, Hpp / bp, the inertial edges' A^T (rho' omega)
template <typename Exec>
SE3_HD void pass_gather(Exec& ex, const Work& F) {
    const liba::Work& W = F.L;
    for (int p = ex.tid(); p < W.P; p += ex.stride()) liba::point_gather(W, p);
    for (int t = ex.tid(); t < 27 * W.Kf; t += ex.stride()) liba::hpp_gather(W, t);
    for (int t = ex.tid(); t < W.NI * kJc * 9; t += ex.stride()) liba::ato_entry(W, t, liba::iedge_active(W, t / (kJc * 9)));
}

// b at copy s
template <typename Exec>
SE3_HD void pass_rhs(Exec& ex, const Work& F, int s) {
    for (int r = ex.tid(); r < F.L.n; r += ex.stride()) F.L.bA[r] = entry_b(F, s, r);
}

// the tasks of `prepare`: [a KeyFrame's own lower triangle | an inertial edge's block between two free KeyFrames | border | corner]
SE3_HD int n_self(const Work& F) { return (places(F) * (places(F) + 1)) / 2; }
SE3_HD long prepare_tasks(const Work& F) {
    const long pl = places(F);
    return (long)F.L.Kf * n_self(F) + (long)F.n_fp * pl * pl + (F.init ? 6L * F.nb + 21 : 0);
}

// One trial's system: Dinv per point, the right side, and H + lambda I written into the CLEARED square S (lower triangle)
template <typename Exec>
SE3_HD void pass_prepare(Exec& ex, const Work& F, double lambda) {
    const liba::Work& W = F.L;
    const int n = W.n, pl = places(F), ns = n_self(F);
    for (int p = ex.tid(); p < W.P; p += ex.stride()) liba::dinv_point(W, p, lambda);
    for (int r = ex.tid(); r < n; r += ex.stride()) W.bs[r] = W.bA[r];
    const long t_self = (long)W.Kf * ns, t_pair = (long)F.n_fp * pl * pl, total = prepare_tasks(F);
    for (long t = ex.tid(); t < total; t += ex.stride()) {
        if (t < t_self) {
            const int i = (int)(t / ns), q = (int)(t % ns);
            int a = 0;                                   // q-th entry of the lower triangle: row a, column b
            while ((a + 1) * (a + 2) / 2 <= q) a++;
            const int b = q - a * (a + 1) / 2;
            if (a >= places(F, i)) continue;             // a KeyFrame without inertial vertices: its pose block alone
            const int r = unknown_at(F, i, a), c = unknown_at(F, i, b);   // (a >= b gives r >= c)
            const double v = entry_self(F, i, a, b);
            W.S[(size_t)r * n + c] = r == c ? v + lambda : v;
        } else if (t < t_self + t_pair) {
            const long q = t - t_self;
            const int m = F.fp_edge[q / (pl * pl)], ua = (int)(q % (pl * pl)) / pl, ub = (int)(q % (pl * pl)) % pl;
            const int ka = W.ie[m].pre.kf_prev, kb = W.ie[m].pre.kf_cur;
            const int ra = unknown_at(F, W.free_of_kf[ka], ua), rb = unknown_at(F, W.free_of_kf[kb], ub);
            if (ra > rb) W.S[(size_t)ra * n + rb] = liba::iedge_entry(W, m, kb, ub, ka, ua);
            else W.S[(size_t)rb * n + ra] = liba::iedge_entry(W, m, ka, ua, kb, ub);
        } else {
            const long q = t - t_self - t_pair;
            if (q < 6L * F.nb) {
                const int j = (int)(q / F.nb), c = (int)(q % F.nb);
                int i, u;
                unknown_of(F, c, i, u);
                W.S[(size_t)(F.nb + j) * n + c] = entry_border(F, i, u, j);
            } else {
                const int z = (int)(q - 6L * F.nb);
                int a = 0;
                while ((a + 1) * (a + 2) / 2 <= z) a++;
                const int b = z - a * (a + 1) / 2;
                const double v = entry_corner(F, a, b);
                W.S[(size_t)(F.nb + a) * n + F.nb + b] = a == b ? v + lambda : v;
            }
        }
    }
}

// the Schur complement over the plan's lists into the pose corner and the poses' right side
template <typename Exec>
SE3_HD void pass_schur(Exec& ex, const Work& F) {
    const int n_tasks = 6 * (F.L.n_pairs + F.L.Kf);
    for (int t = ex.tid(); t < n_tasks; t += ex.stride()) liba::schur_task(F.L, t);
}

// SparseOptimizer::update of copy `from` into copy `to`, and computeScale's terms per vertex
template <typename Exec>
SE3_HD void pass_update(Exec& ex, const Work& F, int from, int to, double lambda) {
    const liba::Work& W = F.L;
    const int n_kf_items = F.init ? W.K : W.Kf;          // init: every KeyFrame's copy of the shared pair moves
    for (int v = ex.tid(); v < n_kf_items + W.P + 1; v += ex.stride()) {
        if (v < n_kf_items) {
            const int k = F.init ? v : W.kf_of_free[v], i = W.free_of_kf[k];
            double u[15];
            for (int a = 0; a < 15; a++) u[a] = 0.0;
            if (F.init)
                for (int j = 0; j < 6; j++) u[9 + j] = W.x[F.nb + j];
            Vertices V = W.st[from][k];
            if (i >= 0) {
                double sc = 0;
                for (int a = 0; a < places(F, i); a++) {
                    const int r = unknown_at(F, i, a);
                    u[a] = W.x[r];
                    sc += u[a] * (lambda * u[a] + W.bA[r]);
                }
                pinert::vertices_update(V, u, W.kf[k].Rcb, W.kf[k].tcb);
                W.part_vtx[i] = sc;
            } else {
                for (int a = 0; a < 3; a++) { V.bg[a] += u[9 + a]; V.ba[a] += u[12 + a]; }
            }
            W.st[to][k] = V;
        } else if (v < n_kf_items + W.P) {
            const int p = v - n_kf_items;
            liba::point_update(W, from, to, lambda, p, W.Kf + p);
        } else {
            double sc = 0;
            if (F.init)
                for (int j = 0; j < 6; j++) sc += W.x[F.nb + j] * (lambda * W.x[F.nb + j] + W.bA[F.nb + j]);
            W.part_vtx[W.Kf + W.P] = sc;
        }
    }
}

// activeRobustChi2 over the errors last evaluated (the priors at copy s), into res->chi.  ONE group of executors with a barrier.
template <typename Exec>
SE3_HD void group_cost(Exec& ex, const Work& F, int s) {
    const liba::Work& W = F.L;
    liba::slot_sum(ex, W, W.rho0, W.E, W.NI ? W.il[0].cost : nullptr, W.NI, (int)(sizeof(liba::IEdgeLin) / sizeof(double)), F.init ? 1 : 3,
                   &F.res->chi);
    if (F.init && ex.tid() == 0) {
        const Vertices& B = W.st[s][F.bias_kf];
        F.res->chi = (F.res->chi + inertial::prior_chi2(B.ba, F.prior_a)) + inertial::prior_chi2(B.bg, F.prior_g);
    }
    ex.barrier();
}

// computeScale's sum into res->scale
template <typename Exec>
SE3_HD void group_scale(Exec& ex, const Work& F) {
    liba::slot_sum(ex, F.L, F.L.part_vtx, F.L.Kf + F.L.P + 1, nullptr, 0, 0, 0, &F.res->scale);
}

// ---- what the C entry and the host program decide before anything runs

struct Problem {
    int code = 0;                  // 0 accepted, 1 invalid, 2 not handled (capacity)
    std::string why;
    int Kf = 0, n = 0, P = 0, E = 0, n_active = 0;
    std::vector<int> fixed, e_in, e_out, fp_edge, point_of, edge_of;   // point_of / edge_of: the included ones' caller indices
    std::vector<int> inert_of_free, free_of_inert;                      // max_kind = 3 alone (Work::inert_of_free)
    std::vector<uint8_t> included;                                      // [n_points]
    std::vector<int> ekf, ept;                                          // the included edges, points renumbered
    LocalBaPlan plan;
};

inline void refuse(Problem& q, int code, const char* why) { q.code = code; q.why = why; }

// The graph of one call.  A point none of whose edges ends at a free KeyFrame is no vertex and its edges do not count
// (Optimizer.cc:677-680); the inertial edges must be chains.
//
// max_kind = 3 (MergeInertialBA): kind 3 is a free pose without inertial vertices, 6 unknowns; a free KeyFrame that no active edge
// reaches is no vertex (g2o's active set) and is planned as a fixed one: no row, its output repeats its input; the capacity is the
// number of unknowns.
inline void plan_problem(int init, int K, const msorb_iba_keyframe* kfs, int NI, const msorb_iba_inertial_edge* ie, int n_points, int n_edges,
                         const int* edge_kf, const int* edge_point, Problem& q, int max_kind = 2) {
    q = Problem();
    q.fixed.resize((size_t)K);
    for (int k = 0; k < K; k++) {
        if (kfs[k].kind < 0 || kfs[k].kind > max_kind)
            return refuse(q, 1, max_kind == 2 ? "an unknown kind (0 free, 1 fixed with inertial vertices, 2 fixed pose)"
                                              : "an unknown kind (0 free, 1 fixed with inertial vertices, 2 fixed pose, 3 free pose only)");
        q.fixed[k] = kfs[k].kind != 0 && kfs[k].kind != 3;
    }
    q.e_in.assign((size_t)K, -1);
    q.e_out.assign((size_t)K, -1);
    bool chains = true;
    for (int i = 0; i < NI; i++) {
        const int a = ie[i].pre.kf_prev, b = ie[i].pre.kf_cur;
        if (a < 0 || a >= K || b < 0 || b >= K) return refuse(q, 1, "an inertial edge names a KeyFrame out of range");
        if (a == b) return refuse(q, 1, "an inertial edge from a KeyFrame to itself");
        if (kfs[a].kind >= 2 || kfs[b].kind >= 2) return refuse(q, 1, "an inertial edge on a KeyFrame without inertial vertices (kind 2 or 3)");
        if (q.e_out[a] >= 0 || q.e_in[b] >= 0) chains = false;
        q.e_out[a] = i;
        q.e_in[b] = i;
    }
    for (int e = 0; e < n_edges; e++) {
        if (edge_kf[e] < 0 || edge_kf[e] >= K || edge_point[e] < 0 || edge_point[e] >= n_points)
            return refuse(q, 1, "an edge names a KeyFrame or a point out of range");
        if (e > 0 && edge_point[e] < edge_point[e - 1]) return refuse(q, 1, "the edges are not point-major");
    }
    if (chains) {   // no cycle: every edge is reached from a KeyFrame that has no incoming one
        int reached = 0;
        for (int k = 0; k < K; k++)
            if (q.e_in[k] < 0)
                for (int m = q.e_out[k]; m >= 0; m = q.e_out[ie[m].pre.kf_cur]) reached++;
        chains = reached == NI;
    }
    if (!chains) return refuse(q, 2, "the inertial edges do not form chains (one incoming and one outgoing edge per KeyFrame)");
    if (max_kind == 3) {
        std::vector<uint8_t> reached((size_t)K, 0);
        for (int e = 0; e < n_edges; e++) reached[edge_kf[e]] = 1;
        for (int i = 0; i < NI; i++) reached[ie[i].pre.kf_prev] = reached[ie[i].pre.kf_cur] = 1;
        for (int k = 0; k < K; k++)
            if (!reached[k]) q.fixed[k] = 1;
    }
    int Ki = 0;
    for (int k = 0; k < K; k++) {
        if (q.fixed[k]) continue;
        q.Kf++;
        if (max_kind == 3) {
            q.inert_of_free.push_back(kfs[k].kind == 0 ? Ki : -1);
            if (kfs[k].kind == 0) { q.free_of_inert.push_back(q.Kf - 1); Ki++; }
        }
    }
    if (max_kind == 3) {
        q.n = 6 * q.Kf + 9 * Ki;
        if (q.n > kMaxN) return refuse(q, 2, "more unknowns than msorb_merge_inertial_ba_capacity()");
    } else {
        if (q.Kf > capacity(init)) return refuse(q, 2, "more free KeyFrames than msorb_full_inertial_ba_capacity()");
        q.n = init ? 9 * q.Kf + 6 : 15 * q.Kf;
    }
    q.included.assign((size_t)n_points, 0);
    for (int e = 0; e < n_edges; e++)
        if (!q.fixed[edge_kf[e]]) q.included[edge_point[e]] = 1;
    std::vector<int> new_of((size_t)n_points, -1);
    for (int p = 0; p < n_points; p++)
        if (q.included[p]) { new_of[p] = (int)q.point_of.size(); q.point_of.push_back(p); }
    for (int e = 0; e < n_edges; e++)
        if (q.included[edge_point[e]]) { q.edge_of.push_back(e); q.ekf.push_back(edge_kf[e]); q.ept.push_back(new_of[edge_point[e]]); }
    q.P = (int)q.point_of.size();
    q.E = (int)q.edge_of.size();
    build_local_ba_plan(K, q.fixed.data(), q.P, q.E, q.ekf.data(), q.ept.data(), q.plan);
    for (int i = 0; i < NI; i++) {
        const bool fa = !q.fixed[ie[i].pre.kf_prev], fb = !q.fixed[ie[i].pre.kf_cur];
        if (fa && fb) q.fp_edge.push_back(i);
        q.n_active += (init || fa || fb) ? 1 : 0;
    }
    q.n_active += q.E + (init ? 2 : 0);
}

// an inertial edge as the device reads it: the random walks' informations are no part of the init form
inline msorb_iba_inertial_edge staged_edge(const msorb_iba_inertial_edge& in, int init) {
    msorb_iba_inertial_edge e = liba::staged_edge(in);
    if (init)
        for (int q = 0; q < 9; q++) e.info_gyro[q] = e.info_acc[q] = 0.0;
    return e;
}

// the state a call starts from; init: every KeyFrame's copy of the shared pair
inline void initial_vertices(Vertices& V, const msorb_iba_keyframe& k, const msorb_fiba_problem& p) {
    liba::vertices_from(V, k);
    if (p.init)
        for (int a = 0; a < 3; a++) { V.bg[a] = p.bg0[a]; V.ba[a] = p.ba0[a]; }
}

// what a KeyFrame's output holds: a free one its estimate; a fixed one its input, and with init and inertial vertices the shared pair
inline void keyframe_result(const msorb_iba_keyframe& in, const Vertices& est, int init, msorb_iba_keyframe_out& o) {
    Vertices V;
    liba::vertices_from(V, in);
    if (in.kind == 0) V = est;
    else if (init && in.kind == 1)
        for (int a = 0; a < 3; a++) { V.bg[a] = est.bg[a]; V.ba[a] = est.ba[a]; }
    liba::keyframe_out(V, o);
}

}  // namespace fiba
}  // namespace msorb
