// ms-slam_amd/csrc/essential_graph4_device.h (the text the kernels compile) and essential_graph_plan.h on the host, serially: every
// sum walks its index list in ascending position, the dense system is factored column by column (L D L^T, no pivoting, one
// reciprocal per pivot: what ldlt_blocked.h is bit-equal to).
//
//   essential_graph4_main in.bin out.bin
// The two files are tests/essential_graph4_cases.py's write_scenes / read_results.  The last column of the printed line is the
// wall time of the optimisation alone, which tools/essential_graph4_latency.py reads.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../ms-slam_amd/csrc/essential_graph4_device.h"
#include "../ms-slam_amd/csrc/essential_graph_plan.h"

using namespace msorb::eg4;

namespace {

constexpr int kVertex = 36;   // Rcw[9] tcw[3] Rwb[9] twb[3] Rcb[9] tcb[3]

struct HostBackend {
    const msorb::EssentialGraphPlan& plan;
    const int *v0, *v1;
    const double *vtx, *meas;
    std::vector<double> state[2], lin, chi, Hd, Hp, b, S, x;
    double tab[kTable * 9];
    int current = 0;
    double max_diagonal = 0;

    void constants(int k, const double** c) const { c[0] = vtx + kVertex * (size_t)k + 12; c[1] = c[0] + 12; c[2] = c[0] + 21; }
    double cost() const {
        double c = 0;
        for (int a = 0; a < plan.Ea; a++) c += chi[a];
        return c;
    }
    int linearise(int cur, double& out) {
        const size_t Ea = (size_t)plan.Ea;
        const std::vector<double>& st = state[cur];
        for (int a = 0; a < plan.Ea; a++) {
            const int e = plan.active_edge[a], i0 = v0[e], i1 = v1[e];
            const bool free0 = plan.free_of_vertex[i0] >= 0, free1 = plan.free_of_vertex[i1] >= 0;
            const double *c0[3], *c1[3];
            constants(i0, c0);
            constants(i1, c1);
            double err[kErrors * 6] = {0}, J[48] = {0};
            for (int w = 0; w < kErrors; w++)
                if (w == 0 || (w < 9 ? free0 : free1))
                    edge_error_variant(tab, meas + 12 * (size_t)e, &st[kState * (size_t)i0], c0, &st[kState * (size_t)i1], c1, w, err + 6 * w);
            chi[a] = edge_chi2(err);
            for (int q = 0; q < 48; q++)
                if (q / 24 ? free1 : free0) J[q] = jacobian_entry(err, q / 24, (q % 24) / 4, q % 4);
            for (int q = 0; q < kPlanes; q++) {
                const bool uses0 = q < kHbb || (q >= kHab && q < kBb), uses1 = (q >= kHbb && q < kBa) || q >= kBb;
                if ((uses0 && !free0) || (uses1 && !free1)) continue;
                lin[(size_t)q * Ea + a] = quadratic_term(J, err, q);
            }
        }
        max_diagonal = 0;
        for (int i = 0; i < plan.Kf; i++) {
            double s[14] = {0};
            for (int m = plan.inc_begin[i]; m < plan.inc_begin[i + 1]; m++) {
                const int a = plan.inc_entry[m] >> 1, side = plan.inc_entry[m] & 1;
                for (int q = 0; q < 10; q++) s[q] += lin[(size_t)((side ? kHbb : kHaa) + q) * Ea + a];
                for (int q = 0; q < 4; q++) s[10 + q] += lin[(size_t)((side ? kBb : kBa) + q) * Ea + a];
            }
            for (int q = 0; q < 10; q++) Hd[10 * (size_t)i + q] = s[q];
            for (int q = 0; q < 4; q++) {
                b[4 * (size_t)i + q] = s[10 + q];
                max_diagonal = std::fmax(std::fabs(s[upper4(q, q)]), max_diagonal);
            }
        }
        for (size_t p = 0; p < plan.pair_i.size(); p++) {
            double t[16] = {0};
            for (int m = plan.pair_begin[p]; m < plan.pair_begin[p + 1]; m++) {
                const int a = plan.pair_entry[m] >> 1, flip = plan.pair_entry[m] & 1;
                for (int r = 0; r < 4; r++)
                    for (int c = 0; c < 4; c++) t[4 * r + c] += lin[(size_t)(kHab + (flip ? 4 * c + r : 4 * r + c)) * Ea + a];
            }
            for (int q = 0; q < 16; q++) Hp[16 * p + q] = t[q];
        }
        out = cost();
        return 0;
    }
    bool solve(int n) {   // column by column; false on a pivot !(d > 0), x untouched
        std::vector<double> v((size_t)n), rd((size_t)n), y(b);
        for (int j = 0; j < n; j++) {
            const double d = S[(size_t)j * n + j];
            if (!(d > 0)) return false;
            const double r = 1.0 / d;
            rd[j] = r;
            for (int i = j + 1; i < n; i++) { v[i] = S[(size_t)i * n + j]; S[(size_t)i * n + j] = v[i] * r; }
            for (int i = j + 1; i < n; i++) {
                const double l = S[(size_t)i * n + j];
                if (l == 0.0) continue;   // (a zero multiplier changes no bit of a finite row)
                for (int k = j + 1; k <= i; k++) S[(size_t)i * n + k] -= l * v[k];
            }
        }
        for (int m = 0; m < n; m++)
            for (int i = m + 1; i < n; i++) y[i] -= S[(size_t)i * n + m] * y[m];
        for (int i = 0; i < n; i++) y[i] *= rd[i];
        for (int m = n - 1; m >= 0; m--)
            for (int i = 0; i < m; i++) y[i] -= S[(size_t)m * n + i] * y[m];
        x = y;
        return true;
    }
    int trial(int cur, double lambda, double& out, double& scale, int& solved) {
        const int n = 4 * plan.Kf;
        std::fill(S.begin(), S.end(), 0.0);
        for (int i = 0; i < plan.Kf; i++)
            for (int r = 0; r < 4; r++)
                for (int c = 0; c <= r; c++) S[(size_t)(4 * i + r) * n + 4 * i + c] = Hd[10 * (size_t)i + upper4(c, r)] + (r == c ? lambda : 0.0);
        for (size_t p = 0; p < plan.pair_i.size(); p++)
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) S[(size_t)(4 * plan.pair_j[p] + c) * n + 4 * plan.pair_i[p] + r] = Hp[16 * p + 4 * r + c];
        solved = solve(n) ? 1 : 0;
        state[cur ^ 1] = state[cur];
        scale = 0;
        for (int i = 0; i < plan.Kf; i++) {
            const int k = plan.vertex_of_free[i];
            const double* u = &x[4 * (size_t)i];
            const double* c[3];
            constants(k, c);
            double dR[9], sc = 0;
            exp_so3(0.0, 0.0, u[0], dR);
            update_w(&state[cur][kState * (size_t)k], dR, u + 1, c[0], c[1], c[2], &state[cur ^ 1][kState * (size_t)k]);
            for (int r = 0; r < 4; r++) sc += u[r] * (lambda * u[r] + b[4 * (size_t)i + r]);
            scale += sc;
        }
        const std::vector<double>& st = state[cur ^ 1];
        for (int a = 0; a < plan.Ea; a++) {
            const int e = plan.active_edge[a];
            const double *s0 = &st[kState * (size_t)v0[e]], *s1 = &st[kState * (size_t)v1[e]];
            double err[6];
            edge_error(s0 + kRcw, s0 + kTcw, s1 + kRcw, s1 + kTcw, meas + 12 * (size_t)e, err);
            chi[a] = edge_chi2(err);
        }
        out = cost();
        return 0;
    }
};

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int n_scenes = 0;
    if (!read_exact(in, &n_scenes, 4)) return 2;
    for (int sidx = 0; sidx < n_scenes; sidx++) {
        int dims[3];
        if (!read_exact(in, dims, 12)) return 2;
        const int N = dims[0], E = dims[1], iterations = dims[2];
        std::vector<double> vtx((size_t)N * kVertex), meas((size_t)E * 12);
        std::vector<int> fixed((size_t)N), v0((size_t)E), v1((size_t)E);
        if (!read_exact(in, vtx.data(), vtx.size() * 8) || !read_exact(in, fixed.data(), (size_t)N * 4) ||
            !read_exact(in, v0.data(), (size_t)E * 4) || !read_exact(in, v1.data(), (size_t)E * 4) || !read_exact(in, meas.data(), meas.size() * 8))
            return 2;
        msorb::EssentialGraphPlan plan;
        if (msorb::build_essential_graph_plan(N, fixed.data(), E, v0.data(), v1.data(), plan) != msorb::kEgPlanOk) return 3;
        const size_t n = 4 * (size_t)plan.Kf, Ea = (size_t)plan.Ea;
        HostBackend be{plan, v0.data(), v1.data(), vtx.data(), meas.data()};
        be.state[0].assign((size_t)N * kState, 0.0);
        for (int k = 0; k < N; k++) {
            const double* v = &vtx[kVertex * (size_t)k];
            state_init(v, v + 9, v + 21, &be.state[0][kState * (size_t)k]);
        }
        be.state[1] = be.state[0];
        be.lin.assign(kPlanes * Ea, 0.0);
        be.chi.assign(Ea, 0.0);
        be.Hd.assign(10 * (size_t)plan.Kf, 0.0);
        be.Hp.assign(16 * plan.pair_i.size(), 0.0);
        be.b.assign(n, 0.0);
        be.S.assign(n * n, 0.0);
        be.x.assign(n, 0.0);
        for (int k = 0; k < kTable; k++) exp_so3(0.0, 0.0, k == 0 ? 1e-9 : k == 1 ? -1e-9 : 0.0, be.tab + 9 * k);
        msorb::eg::Outcome o;
        const auto t0 = std::chrono::steady_clock::now();
        if (msorb::eg::levenberg(be, iterations, plan.Ea > 0, o, [](HostBackend& h) { return lambda_init(h.max_diagonal); })) return 4;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        const int counts[6] = {0, o.iterations, o.trials, o.rejected, o.solver_failures, o.stop};
        const double d[4] = {o.chi2_initial, o.chi2_final, o.lambda, o.lambda_initial};
        std::fwrite(counts, 4, 6, out);
        std::fwrite(d, 8, 4, out);
        std::vector<double> result((size_t)N * 12);   // a vertex outside the system repeats its input
        for (int k = 0; k < N; k++) std::memcpy(&result[12 * (size_t)k], &vtx[kVertex * (size_t)k], 96);
        for (int i = 0; i < plan.Kf; i++) {
            const int k = plan.vertex_of_free[i];
            std::memcpy(&result[12 * (size_t)k], &be.state[be.current][kState * (size_t)k + kRcw], 96);
        }
        std::fwrite(result.data(), 8, result.size(), out);
        std::printf("scene %d: N %d free %d edges %d active %d pairs %zu iterations %d trials %d rejected %d stop %d chi2 %.6e -> %.6e ms %.3f\n", sidx, N,
                    plan.Kf, E, plan.Ea, plan.pair_i.size(), o.iterations, o.trials, o.rejected, o.stop, o.chi2_initial, o.chi2_final, ms);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
