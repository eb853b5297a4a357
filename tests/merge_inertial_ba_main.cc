// ms-slam_amd/csrc/merge_inertial_ba_device.h (the text the kernels compile) on the host, serially: one executor walks every item of
// every pass in ascending order, the reduced system is solved column by column (liba::solve, the arithmetic the blocked solve
// repeats bit for bit), and eg::levenberg, the loop the C entry runs, drives it from lambda 1e3.
//
//   merge_inertial_ba_main in.bin out.bin    the scenes of tests/merge_inertial_ba_cases.py's write_scenes -> read_results
// in:  int32 n_scenes, then per scene int32 iterations, K, NI, P, E, stop_after_trials, stop_before_iteration (-1 = never), 0, then
//      msorb_iba_keyframe [K], msorb_iba_inertial_edge [NI], pos_w [3 P] floats, edge_kf [E], edge_point [E] int32, xy [2 E],
//      u_right [E], inv_sigma2 [E] floats.
// out: per scene msorb_iba_result, msorb_iba_keyframe_out [K], the points [3 P] doubles, point_included [P], edge_outlier [E].
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../ms-slam_amd/csrc/merge_inertial_ba_device.h"

using namespace msorb::miba;
namespace fiba = msorb::fiba;
namespace liba = msorb::liba;

namespace {

struct SerialExec {
    int tid() const { return 0; }
    int stride() const { return 1; }
    void barrier() {}
};

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

struct Backend {
    Work F;
    Res res;
    int current = 0;
    int linearise(int cur, double& chi) {
        SerialExec ex;
        fiba::pass_edges<true>(ex, F, cur);
        fiba::pass_gather(ex, F);
        fiba::pass_rhs(ex, F, cur);
        fiba::group_cost(ex, F, cur);
        chi = res.chi;
        return 0;
    }
    int trial(int cur, double lambda, double& chi, double& scale, int& solved) {
        SerialExec ex;
        const liba::Work& W = F.L;
        std::memset(W.S, 0, (size_t)W.n * W.n * 8);
        fiba::pass_prepare(ex, F, lambda);
        fiba::pass_schur(ex, F);
        solved = liba::solve(ex, W) ? 1 : 0;
        fiba::pass_update(ex, F, cur, cur ^ 1, lambda);
        fiba::pass_edges<false>(ex, F, cur ^ 1);
        fiba::group_cost(ex, F, cur ^ 1);
        fiba::group_scale(ex, F);
        chi = res.chi;
        scale = res.scale;
        return 0;
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int n_scenes = 0;
    if (!read_exact(in, &n_scenes, 4)) return 2;
    for (int sidx = 0; sidx < n_scenes; sidx++) {
        int hd[8];
        if (!read_exact(in, hd, sizeof hd)) return 2;
        const int iterations = hd[0], K = hd[1], NI = hd[2], NP = hd[3], NE = hd[4], stop_trials = hd[5], stop_iteration = hd[6];
        if (K < 0 || NI < 0 || NP < 0 || NE < 0) return 2;
        std::vector<msorb_iba_keyframe> kfs((size_t)K);
        std::vector<msorb_iba_inertial_edge> ie((size_t)NI);
        std::vector<float> pos(3 * (size_t)NP), xy_in(2 * (size_t)NE), ur_in((size_t)NE), inv_in((size_t)NE);
        std::vector<int> ekf((size_t)NE), ept((size_t)NE);
        if (!read_exact(in, kfs.data(), kfs.size() * sizeof(kfs[0])) || !read_exact(in, ie.data(), ie.size() * sizeof(ie[0])) ||
            !read_exact(in, pos.data(), 12 * (size_t)NP) || !read_exact(in, ekf.data(), 4 * (size_t)NE) ||
            !read_exact(in, ept.data(), 4 * (size_t)NE) || !read_exact(in, xy_in.data(), 8 * (size_t)NE) ||
            !read_exact(in, ur_in.data(), 4 * (size_t)NE) || !read_exact(in, inv_in.data(), 4 * (size_t)NE))
            return 2;
        Problem q;
        plan_problem(K, kfs.data(), NI, ie.data(), NP, NE, ekf.data(), ept.data(), q);
        if (q.code) { std::printf("scene %d refused: %s\n", sidx, q.why.c_str()); return 3; }
        for (int i = 0; i < NI; i++) ie[i] = liba::staged_edge(ie[i]);
        const msorb::LocalBaPlan& plan = q.plan;
        const int Kf = q.Kf, n = q.n, P = q.P, E = q.E;
        std::vector<float> xy(2 * (size_t)E), ur((size_t)E), inv((size_t)E);
        for (int e = 0; e < E; e++) {
            xy[2 * (size_t)e] = xy_in[2 * (size_t)q.edge_of[e]];
            xy[2 * (size_t)e + 1] = xy_in[2 * (size_t)q.edge_of[e] + 1];
            ur[e] = ur_in[q.edge_of[e]];
            inv[e] = inv_in[q.edge_of[e]];
        }
        std::vector<Vertices> st0((size_t)K), st1;
        std::vector<double> pt0(3 * (size_t)P), pt1;
        for (int k = 0; k < K; k++) { std::memset(static_cast<void*>(&st0[k]), 0, sizeof(Vertices)); liba::vertices_from(st0[k], kfs[k]); }
        for (int i = 0; i < P; i++)
            for (int a = 0; a < 3; a++) pt0[3 * (size_t)i + a] = (double)pos[3 * (size_t)q.point_of[i] + a];
        st1 = st0;
        pt1 = pt0;
        std::vector<double> lin((size_t)liba::kPlanes * E), Hpp((size_t)Kf * 27), Hll((size_t)P * 9), Dinv((size_t)P * 9), bA((size_t)n), S((size_t)n * n),
            bs((size_t)n), x((size_t)n, 0.0), cv((size_t)n), cl((size_t)n), y((size_t)n), rd((size_t)n), chi2((size_t)E, 0.0), rho0((size_t)E),
            slots((size_t)liba::kSlots), pv((size_t)Kf + P + 1);
        std::vector<liba::IEdgeLin> il((size_t)NI);
        if (NI) std::memset(static_cast<void*>(il.data()), 0, il.size() * sizeof(liba::IEdgeLin));
        Backend be{};
        Work& F = be.F;
        liba::Work& W = F.L;
        W.K = K; W.Kf = Kf; W.P = P; W.E = E; W.NI = NI; W.n = n; W.n_pairs = (int)plan.pair_i.size();
        W.shared_bias = 0;
        W.kf = kfs.data(); W.ie = ie.data();
        W.free_of_kf = plan.free_of_kf.data(); W.kf_of_free = plan.kf_of_free.data(); W.edge_kf = q.ekf.data(); W.edge_pt = q.ept.data();
        W.point_begin = plan.point_begin.data(); W.kf_begin = plan.kf_begin.data(); W.kf_edge = plan.kf_edge.data();
        W.pair_begin = plan.pair_begin.data(); W.pair_i = plan.pair_i.data(); W.pair_j = plan.pair_j.data(); W.pair_a = plan.pair_a.data();
        W.pair_b = plan.pair_b.data(); W.e_in = q.e_in.data(); W.e_out = q.e_out.data();
        W.xy = xy.data(); W.ur = ur.data(); W.w = inv.data();
        W.st[0] = st0.data(); W.st[1] = st1.data(); W.pt[0] = pt0.data(); W.pt[1] = pt1.data();
        W.lin = lin.data(); W.Hpp = Hpp.data(); W.Hll = Hll.data(); W.Dinv = Dinv.data(); W.bA = bA.data(); W.S = S.data();
        W.bs = bs.data(); W.x = x.data(); W.col_v = cv.data(); W.col_l = cl.data(); W.y = y.data(); W.rd = rd.data(); W.chi2 = chi2.data();
        W.rho0 = rho0.data(); W.slots = slots.data(); W.part_vtx = pv.data(); W.il = il.data();
        F.init = 0; F.per = 9; F.nb = n; F.n_fp = (int)q.fp_edge.size(); F.fp_edge = q.fp_edge.data();
        F.inert_of_free = q.inert_of_free.data(); F.free_of_inert = q.free_of_inert.data();
        F.res = &be.res;
        msorb_iba_result R;
        std::memset(&R, 0, sizeof R);
        const auto t0 = std::chrono::steady_clock::now();
        msorb::eg::Outcome o{};
        if (Kf == 0) R.status = 2;
        else if (stop_trials == 0 || stop_iteration == 0) R.status = 3;           // the flag is set before optimize()
        else {
            msorb::eg::levenberg(be, iterations > 0 ? iterations : kIterations, q.n_active > 0, o, [](Backend&) { return kLambdaInit; }, [&] {
                return (stop_trials >= 0 && o.trials >= stop_trials) || (stop_iteration >= 0 && o.iterations >= stop_iteration);
            });
            if (o.iterations == 0) R.status = 3;                                  // it rose before the first iteration: handed back
            else {
                R.iterations = o.iterations; R.trials = o.trials; R.rejected_trials = o.rejected;
                R.reserved = o.solver_failures; R.chi2_initial = o.chi2_initial; R.chi2_final = o.chi2_final; R.lambda_final = o.lambda;
            }
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        const int cur = be.current;
        std::vector<msorb_iba_keyframe_out> ko((size_t)K);
        std::vector<double> pts(3 * (size_t)NP);
        std::vector<uint8_t> inc((size_t)NP, 0), flags((size_t)NE, 0), outlier((size_t)E, 0);
        for (size_t i = 0; i < pts.size(); i++) pts[i] = (double)pos[i];
        for (int k = 0; k < K; k++) {
            std::memset(&ko[k], 0, sizeof ko[k]);
            keyframe_result(kfs[k], R.status ? -1 : plan.free_of_kf[k], W.st[cur][k], ko[k]);
        }
        if (!R.status) {
            SerialExec ex;
            pass_classify(ex, F, outlier.data());
            for (int e = 0; e < E; e++) { flags[q.edge_of[e]] = outlier[e]; R.n_outliers += outlier[e]; }
            for (int i = 0; i < P; i++)
                for (int a = 0; a < 3; a++) pts[3 * (size_t)q.point_of[i] + a] = W.pt[cur][3 * (size_t)i + a];
            for (int i = 0; i < NP; i++) inc[i] = q.included[i];
        }
        std::fwrite(&R, sizeof R, 1, out);
        if (K) std::fwrite(ko.data(), sizeof ko[0], (size_t)K, out);
        if (NP) std::fwrite(pts.data(), 8, 3 * (size_t)NP, out);
        if (NP) std::fwrite(inc.data(), 1, (size_t)NP, out);
        if (NE) std::fwrite(flags.data(), 1, (size_t)NE, out);
        std::printf("scene %d: Kf %d K %d NI %d P %d/%d E %d/%d n %d status %d iterations %d trials %d rejected %d flagged %d chi2 %.17g -> %.17g in %.3f ms\n",
                    sidx, Kf, K, NI, P, NP, E, NE, n, R.status, R.iterations, R.trials, R.rejected_trials, R.n_outliers, R.chi2_initial, R.chi2_final, ms);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
