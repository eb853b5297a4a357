// ms-slam_amd/csrc/pose_rig_device.h, the edge functions the rig kernel of pose_opt.hip compiles, built for the host and run serially:
// the whole of Optimizer::PoseOptimization's two-camera arm (src/Optimizer.cc:870-1037 with g2o's Levenberg loop) over those edges,
// summed in forward order.  The loop below is this program's own (the kernel's is device code); the edges are the header's.  No GPU,
// no library: g++ -std=c++17 -O2 -ffp-contract=off tests/pose_opt_rig_main.cc.
//
//   pose_opt_rig_main solve in.bin out.bin
//     in : msorb_pose_rig_problem | xy [2n float] | camera [n uint8] | inv_sigma2 [n float] | pos_w [3n float]
//     out: msorb_pose_result | outlier [n uint8]
//   pose_opt_rig_main grid in.bin out.bin
//     in : msorb_pose_rig_problem (pose, cameras, Trl; n ignored) | m (int) | Xw [3m double] | camera [m uint8]
//     out: per point 14 doubles: the edge's error with a zero observation (= -project) e[2], its Jacobian J[2][6]
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/msorb.h"
#include "../ms-slam_amd/csrc/pose_rig_device.h"

using namespace msorb::se3;
namespace rig = msorb::rig;

namespace {

// L D L^T of H + lambda I without pivoting, one reciprocal per pivot (as the kernel and tests/pose_opt_cases.py solve it)
bool solve6(const double* Hu, double lambda, const double* b, double* x) {
    double L[6][6], r[6];
    int k = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) { L[j][i] = Hu[k++]; if (i == j) L[i][i] += lambda; }
    for (int j = 0; j < 6; j++) {
        double v[6];
        double d = L[j][j];
        for (int m = 0; m < j; m++) { v[m] = L[j][m] * L[m][m]; d -= L[j][m] * v[m]; }
        if (!(d > 0)) return false;
        L[j][j] = d;
        r[j] = 1.0 / d;
        for (int i = j + 1; i < 6; i++) {
            double s = L[i][j];
            for (int m = 0; m < j; m++) s -= L[i][m] * v[m];
            L[i][j] = s * r[j];
        }
    }
    double y[6];
    for (int i = 0; i < 6; i++) {
        double s = b[i];
        for (int m = 0; m < i; m++) s -= L[i][m] * y[m];
        y[i] = s;
    }
    for (int i = 5; i >= 0; i--) {
        double s = y[i] * r[i];
        for (int m = i + 1; m < 6; m++) s -= L[m][i] * x[m];
        x[i] = s;
    }
    return true;
}

rig::Rig make_rig(const msorb_pose_rig_problem& p) {
    rig::Rig g;
    for (int c = 0; c < 2; c++) {
        g.cam[c].type = p.cam[c].type;
        for (int k = 0; k < 8; k++) g.cam[c].p[k] = p.cam[c].p[k];
    }
    const float q1[4] = {0, 0, 0, 1}, t1[3] = {0, 0, 0};
    if (p.n_cameras == 2) rig::set_trl(g, p.q_rl, p.t_rl);
    else rig::set_trl(g, q1, t1);
    return g;
}

Pose start_pose(const msorb_pose_rig_problem& p) {   // Optimizer.cc:774-775
    Pose T{(double)p.q[0], (double)p.q[1], (double)p.q[2], (double)p.q[3], (double)p.t[0], (double)p.t[1], (double)p.t[2]};
    normalize_rotation(T);
    return T;
}

struct Edges {
    const rig::Rig& g;
    int n;
    const float *xy, *inv, *pos;
    const uint8_t* camera;
    double error(int i, const Pose& T, const Pose& Trw, double* e, double& x, double& y, double& z) const {
        return rig::edge_error(g, T, Trw, camera[i] != 0, (double)xy[2 * i], (double)xy[2 * i + 1], (double)inv[i], (double)pos[3 * i],
                               (double)pos[3 * i + 1], (double)pos[3 * i + 2], e, x, y, z);
    }
};

void solve(const msorb_pose_rig_problem& p, const Edges& E, msorb_pose_result& R, std::vector<uint8_t>& level) {
    const int n = E.n;
    std::memset(&R, 0, sizeof R);
    for (int k = 0; k < 4; k++) { R.iterations[k] = -1; R.rejected_trials[k] = -1; }
    R.n_initial = n;
    level.assign(n, 0);
    if (n < 3) {   // :936-937
        for (int k = 0; k < 4; k++) { R.q[k] = p.q[k]; R.qd[k] = (double)p.q[k]; }
        for (int k = 0; k < 3; k++) { R.t[k] = p.t[k]; R.td[k] = (double)p.t[k]; }
        R.n_bad = n;
        return;
    }
    const double delta = (double)(float)std::sqrt(5.991);   // deltaMono (:796)
    const Pose T0 = start_pose(p);
    Pose T = T0;
    std::vector<double> chi2(n, 0.0);
    double x[6] = {0, 0, 0, 0, 0, 0};
    int n_bad = 0;
    for (int it = 0; it < 4; it++) {
        const bool robust = it < 3;
        T = T0;
        int n_solve = 0, n_rejected = 0;
        if (n - n_bad > 0) {
            double lambda = 0, ni = 2;
            int n_bad_steps = 0;
            bool ok = true;
            for (int i = 0; i < 10 && ok; i++) {
                double S[28];
                for (double& s : S) s = 0;
                const Pose Trw = rig::compose(E.g.Trl, T);
                for (int k = 0; k < n; k++) {
                    if (level[k]) continue;
                    double e[2], px, py, pz, J[2][6], rho0, rho1;
                    chi2[k] = E.error(k, T, Trw, e, px, py, pz);
                    huber(chi2[k], delta, robust, rho0, rho1);
                    S[27] += rho0;
                    rig::edge_jacobian(E.g, E.camera[k] != 0, px, py, pz, J);
                    const double w = (double)E.inv[k], wr = rho1 * w;
                    int m = 0;
                    for (int a = 0; a < 6; a++) {
                        for (int c = a; c < 6; c++, m++) S[m] += (J[0][a] * wr) * J[0][c] + (J[1][a] * wr) * J[1][c];
                        S[21 + a] -= ((rho1 * J[0][a]) * w) * e[0] + ((rho1 * J[1][a]) * w) * e[1];
                    }
                }
                double current = S[27], temp = current;
                const double ini = current;
                const double* Hu = S;
                const double* b = S + 21;
                if (i == 0) {
                    double max_diag = 0;
                    for (int j = 0, k = 0; j < 6; k += 6 - j, j++) max_diag = std::fmax(std::fabs(Hu[k]), max_diag);
                    lambda = 1e-5 * max_diag;
                    ni = 2;
                    n_bad_steps = 0;
                }
                double rho = 0;
                int qmax = 0;
                do {
                    const Pose backup = T;
                    const bool ok2 = solve6(Hu, lambda, b, x);
                    T = oplus(T, x);
                    const Pose Trw2 = rig::compose(E.g.Trl, T);
                    double c1 = 0;
                    for (int k = 0; k < n; k++) {
                        if (level[k]) continue;
                        double e[2], px, py, pz, rho0, rho1;
                        chi2[k] = E.error(k, T, Trw2, e, px, py, pz);
                        huber(chi2[k], delta, robust, rho0, rho1);
                        c1 += rho0;
                    }
                    temp = c1;
                    if (!ok2) temp = DBL_MAX;
                    rho = current - temp;
                    double scale = 0;
                    for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + b[j]);
                    scale += 1e-3;
                    rho /= scale;
                    if (rho > 0 && std::isfinite(temp)) {
                        const double y = 2 * rho - 1;
                        double alpha = 1. - (y * y) * y;
                        alpha = std::fmin(alpha, 2. / 3.);
                        lambda *= std::fmax(1. / 3., alpha);
                        ni = 2;
                        current = temp;
                    } else {
                        lambda *= ni;
                        ni *= 2;
                        T = backup;
                        n_rejected++;
                    }
                    qmax++;
                } while (rho < 0 && qmax < 10);
                n_solve++;
                if (qmax == 10 || rho == 0) { ok = false; continue; }
                if ((ini - current) * 1e3 < ini) n_bad_steps++;
                else n_bad_steps = 0;
                if (n_bad_steps >= 3) ok = false;
            }
        }
        R.iterations[it] = n_solve;
        R.rejected_trials[it] = n_rejected;
        const Pose Trw = rig::compose(E.g.Trl, T);
        n_bad = 0;
        for (int k = 0; k < n; k++) {
            if (level[k]) {
                double e[2], px, py, pz;
                chi2[k] = E.error(k, T, Trw, e, px, py, pz);
            }
            level[k] = (float)chi2[k] > 5.991f ? 1 : 0;
            n_bad += level[k];
        }
        if (n < 10) break;
    }
    R.qd[0] = T.qx; R.qd[1] = T.qy; R.qd[2] = T.qz; R.qd[3] = T.qw;
    R.td[0] = T.tx; R.td[1] = T.ty; R.td[2] = T.tz;
    for (int k = 0; k < 4; k++) R.q[k] = (float)R.qd[k];
    for (int k = 0; k < 3; k++) R.t[k] = (float)R.td[k];
    R.n_bad = n_bad;
}

template <class T>
bool read_n(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* in = std::fopen(argv[2], "rb");
    if (!in) return 2;
    msorb_pose_rig_problem p;
    if (std::fread(&p, sizeof p, 1, in) != 1) return 2;
    const rig::Rig g = make_rig(p);
    FILE* out = nullptr;
    if (std::strcmp(argv[1], "solve") == 0) {
        std::vector<float> xy, inv, pos;
        std::vector<uint8_t> camera;
        const size_t n = (size_t)p.n;
        if (!read_n(in, xy, 2 * n) || !read_n(in, camera, n) || !read_n(in, inv, n) || !read_n(in, pos, 3 * n)) return 2;
        const Edges E{g, p.n, xy.data(), inv.data(), pos.data(), camera.data()};
        msorb_pose_result R;
        std::vector<uint8_t> level;
        solve(p, E, R, level);
        out = std::fopen(argv[3], "wb");
        if (!out) return 2;
        std::fwrite(&R, sizeof R, 1, out);
        if (n) std::fwrite(level.data(), 1, n, out);
    } else if (std::strcmp(argv[1], "grid") == 0) {
        int m = 0;
        std::vector<double> X;
        std::vector<uint8_t> camera;
        if (std::fread(&m, 4, 1, in) != 1 || m < 0 || !read_n(in, X, 3 * (size_t)m) || !read_n(in, camera, (size_t)m)) return 2;
        const Pose T = start_pose(p);
        const Pose Trw = rig::compose(g.Trl, T);
        out = std::fopen(argv[3], "wb");
        if (!out) return 2;
        for (int i = 0; i < m; i++) {
            double rec[14], x, y, z, J[2][6];
            rig::edge_error(g, T, Trw, camera[i] != 0, 0.0, 0.0, 1.0, X[3 * i], X[3 * i + 1], X[3 * i + 2], rec, x, y, z);
            rig::edge_jacobian(g, camera[i] != 0, x, y, z, J);
            std::memcpy(rec + 2, J, sizeof J);
            std::fwrite(rec, 8, 14, out);
        }
    } else {
        return 2;
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
