// ms-slam_amd/csrc/full_inertial_ba_device.h (the text the kernels compile) on the host, serially: one executor walks every item of
// every pass in ascending order, the reduced system is solved column by column (liba::solve, the arithmetic the blocked solve
// repeats bit for bit), and eg::levenberg, the loop the C entry runs, drives it.
//
//   full_inertial_ba_main in.bin out.bin     the scenes of tests/full_inertial_ba_cases.py's write_scenes -> read_results
//   full_inertial_ba_main --terminate        eg::levenberg with the stop callable on hand-made costs: rho == 0 ends the call after
//                                            one trial, ten rejected trials end it, three iterations that gain too little end it,
//                                            a flag raised after a chosen trial or before a chosen iteration ends it there
// in:  int32 n_scenes, then per scene int32 init, iterations, K, NI, P, E, stop_after_trials, stop_before_iteration (-1 = never),
//      float prior_g, prior_a, double bg0 [3], ba0 [3], then msorb_iba_keyframe [K], msorb_iba_inertial_edge [NI], pos_w [3 P]
//      floats, edge_kf [E], edge_point [E] int32, xy [2 E], u_right [E], inv_sigma2 [E] floats.
// out: per scene msorb_iba_result, msorb_iba_keyframe_out [K], the points [3 P] doubles, point_included [P].
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../ms-slam_amd/csrc/full_inertial_ba_device.h"

using namespace msorb::fiba;
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
        pass_edges<true>(ex, F, cur);
        pass_gather(ex, F);
        pass_rhs(ex, F, cur);
        group_cost(ex, F, cur);
        chi = res.chi;
        return 0;
    }
    int trial(int cur, double lambda, double& chi, double& scale, int& solved) {
        SerialExec ex;
        const liba::Work& W = F.L;
        std::memset(W.S, 0, (size_t)W.n * W.n * 8);
        pass_prepare(ex, F, lambda);
        pass_schur(ex, F);
        solved = liba::solve(ex, W) ? 1 : 0;
        pass_update(ex, F, cur, cur ^ 1, lambda);
        pass_edges<false>(ex, F, cur ^ 1);
        group_cost(ex, F, cur ^ 1);
        group_scale(ex, F);
        chi = res.chi;
        scale = res.scale;
        return 0;
    }
};

// a backend of hand-made costs: every trial offers cost * (1 - gain)
struct Fake {
    double cost, gain;
    int current = 0, last = 0, trials = 0;
    int linearise(int cur, double& chi) {
        if (cur != last) { cost -= gain * cost; last = cur; }   // the loop took the trial: it is the state now
        chi = cost;
        return 0;
    }
    int trial(int, double, double& chi, double& scale, int& solved) { solved = 1; scale = 1.0; trials++; chi = cost - gain * cost; return 0; }
};

int terminate_check() {
    int bad = 0;
    msorb::eg::Outcome o;
    auto init = [](Fake&) { return 1e-5; };
    auto never = [] { return false; };
    Fake a{100.0, 0.0};                                                        // the trial gains nothing: rho == 0
    msorb::eg::levenberg(a, 10, true, o, init, never);
    bad += !(o.iterations == 1 && o.trials == 1 && o.rejected == 1 && o.stop == 1);
    Fake b{100.0, -0.5};                                                       // every trial is worse: ten rejected, lambda 1e-5 2^(1+..+10)
    msorb::eg::levenberg(b, 10, true, o, init, never);
    bad += !(o.iterations == 1 && o.trials == 10 && o.rejected == 10 && o.stop == 1 && o.lambda == 1e-5 * 36028797018963968.0);
    Fake c{100.0, 1e-4};                                                       // accepted, but (ini - current) * 1e3 < ini three times
    msorb::eg::levenberg(c, 10, true, o, init, never);
    bad += !(o.iterations == 3 && o.trials == 3 && o.rejected == 0 && o.stop == 2);
    Fake d{100.0, 0.5};                                                        // plain progress: all seven iterations
    msorb::eg::levenberg(d, 7, true, o, init, never);
    bad += !(o.iterations == 7 && o.trials == 7 && o.rejected == 0 && o.stop == 0 && o.chi2_initial == 100.0);
    Fake e{100.0, 0.5};                                                        // the flag before iteration 3: three iterations made
    msorb::eg::levenberg(e, 7, true, o, init, [&] { return o.iterations >= 3; });
    bad += !(o.iterations == 3 && o.trials == 3 && o.stop == 3 && e.current == 1);
    Fake f{100.0, -0.5};                                                       // the flag after the fourth rejected trial: the loop of
    msorb::eg::levenberg(f, 7, true, o, init, [&] { return f.trials >= 4; });  // trials ends, qmax != 10 and rho != 0, no next iteration
    bad += !(o.iterations == 1 && o.trials == 4 && o.rejected == 4 && o.stop == 3 && f.current == 0 && o.chi2_final == 100.0);
    Fake g{100.0, 0.5};                                                        // set before optimize(): nothing runs
    msorb::eg::levenberg(g, 7, true, o, init, [] { return true; });
    bad += !(o.iterations == 0 && o.trials == 0 && g.trials == 0);
    std::printf("terminate: %d checks differ\n", bad);
    return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--terminate")) return terminate_check();
    if (argc < 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int n_scenes = 0;
    if (!read_exact(in, &n_scenes, 4)) return 2;
    for (int sidx = 0; sidx < n_scenes; sidx++) {
        int hd[8];
        msorb_fiba_problem pr;
        std::memset(&pr, 0, sizeof pr);
        if (!read_exact(in, hd, sizeof hd) || !read_exact(in, &pr.prior_g, 8) || !read_exact(in, pr.bg0, 48)) return 2;
        const int init = hd[0], iterations = hd[1], K = hd[2], NI = hd[3], NP = hd[4], NE = hd[5], stop_trials = hd[6], stop_iteration = hd[7];
        if (K < 0 || NI < 0 || NP < 0 || NE < 0 || (init != 0 && init != 1)) return 2;
        pr.init = init;
        pr.iterations = iterations;
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
        plan_problem(init, K, kfs.data(), NI, ie.data(), NP, NE, ekf.data(), ept.data(), q);
        if (q.code) { std::printf("scene %d refused: %s\n", sidx, q.why.c_str()); return 3; }
        for (int i = 0; i < NI; i++) ie[i] = staged_edge(ie[i], init);
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
        for (int k = 0; k < K; k++) { std::memset(static_cast<void*>(&st0[k]), 0, sizeof(Vertices)); initial_vertices(st0[k], kfs[k], pr); }
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
        W.shared_bias = init;
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
        F.init = init; F.per = init ? 3 : 9; F.nb = 9 * Kf; F.n_fp = (int)q.fp_edge.size(); F.fp_edge = q.fp_edge.data();
        F.prior_g = (double)pr.prior_g; F.prior_a = (double)pr.prior_a;
        F.bias_kf = 0;
        for (int k = 0; k < K; k++)
            if (kfs[k].kind != 2) F.bias_kf = k;
        F.res = &be.res;
        msorb_iba_result R;
        std::memset(&R, 0, sizeof R);
        const auto t0 = std::chrono::steady_clock::now();
        const bool nothing = K == 0 || (!init && Kf == 0);
        msorb::eg::Outcome o{};
        if (nothing) R.status = 2;
        else if (stop_trials == 0 || stop_iteration == 0) R.status = 3;           // the flag is set before optimize()
        else {
            msorb::eg::levenberg(be, iterations, q.n_active > 0, o, [](Backend&) { return 1e-5; }, [&] {
                return (stop_trials >= 0 && o.trials >= stop_trials) || (stop_iteration >= 0 && o.iterations >= stop_iteration);
            });
            R.iterations = o.iterations; R.trials = o.trials; R.rejected_trials = o.rejected;
            R.reserved = o.solver_failures; R.chi2_initial = o.chi2_initial; R.chi2_final = o.chi2_final; R.lambda_final = o.lambda;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        const int cur = be.current;
        std::vector<msorb_iba_keyframe_out> ko((size_t)K);
        std::vector<double> pts(3 * (size_t)NP);
        std::vector<uint8_t> inc((size_t)NP, 0);
        for (size_t i = 0; i < pts.size(); i++) pts[i] = (double)pos[i];
        for (int k = 0; k < K; k++) {
            std::memset(&ko[k], 0, sizeof ko[k]);
            if (R.status) { Vertices V; std::memset(static_cast<void*>(&V), 0, sizeof V); liba::vertices_from(V, kfs[k]); liba::keyframe_out(V, ko[k]); }
            else keyframe_result(kfs[k], W.st[cur][k], init, ko[k]);
        }
        if (!R.status) {
            for (int i = 0; i < P; i++)
                for (int a = 0; a < 3; a++) pts[3 * (size_t)q.point_of[i] + a] = W.pt[cur][3 * (size_t)i + a];
            for (int i = 0; i < NP; i++) inc[i] = q.included[i];
        }
        std::fwrite(&R, sizeof R, 1, out);
        if (K) std::fwrite(ko.data(), sizeof ko[0], (size_t)K, out);
        if (NP) std::fwrite(pts.data(), 8, 3 * (size_t)NP, out);
        if (NP) std::fwrite(inc.data(), 1, (size_t)NP, out);
        std::printf("scene %d: init %d Kf %d K %d NI %d P %d/%d E %d/%d n %d status %d iterations %d trials %d rejected %d chi2 %.17g -> %.17g in %.3f ms\n",
                    sidx, init, Kf, K, NI, P, NP, E, NE, n, R.status, R.iterations, R.trials, R.rejected_trials, R.chi2_initial, R.chi2_final, ms);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
