// ms-slam_amd/csrc/pose_inertial_device.h (the text the kernel compiles) on the host, serially: one executor walks every visual edge
// and every entry of the multi-edges and of the system in ascending order, every sum is added left to right.
//
//   pose_inertial_main in.bin out.bin       the scenes of tests/pose_inertial_cases.py's write_scenes -> read_results
// in:  int32 n_scenes, then per scene msorb_pose_inertial_problem, xy [2 n], u_right [n], inv_sigma2 [n], pos_w [3 n] as floats and
//      close [n] as bytes.
// out: per scene msorb_pose_inertial_result, the flags [n], every edge's chi2 as the routine leaves it [n] (the C ABI does not return
//      it), the 15 singular values Marginalize thresholds (form 1, else zeros) and the 15 eigenvalues ConstraintPoseImu's
//      constructor thresholds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../ms-slam_amd/csrc/pose_inertial_device.h"

using namespace msorb::pinert;

namespace {

struct SerialExec {
    int tid() const { return 0; }
    int stride() const { return 1; }
    void barrier() {}
    bool leads(int) const { return true; }
    void sum(double*, int) {}
};

struct HostObs {
    std::vector<Ob> ob;
    std::vector<double> chi2;
    std::vector<uint8_t> level;
    template <typename F>
    void each(F f) {
        for (size_t i = 0; i < ob.size(); i++) f(ob[i], chi2[i], level[i], (int)i);
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
    std::vector<msorb_pose_inertial_problem> Pv(1);
    std::vector<msorb_pose_inertial_result> Rv(1);
    std::vector<Shared> Sv(1);
    for (int sidx = 0; sidx < n_scenes; sidx++) {
        msorb_pose_inertial_problem& P = Pv[0];
        if (!read_exact(in, &P, sizeof(P)) || P.n < 0) return 2;
        const size_t n = (size_t)P.n;
        std::vector<float> xy(2 * n), ur(n), inv(n), pos(3 * n);
        std::vector<uint8_t> close(n), flags(n);
        if (!read_exact(in, xy.data(), 8 * n) || !read_exact(in, ur.data(), 4 * n) || !read_exact(in, inv.data(), 4 * n) ||
            !read_exact(in, pos.data(), 12 * n) || !read_exact(in, close.data(), n))
            return 2;
        HostObs obs;
        obs.ob.resize(n);
        obs.chi2.assign(n, 0.0);
        obs.level.assign(n, 0);
        for (size_t i = 0; i < n; i++)
            obs.ob[i] = Ob{xy[2 * i], xy[2 * i + 1], ur[i], inv[i], pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], close[i] != 0};
        msorb_pose_inertial_result& R = Rv[0];
        std::memset(&R, 0, sizeof(R));
        std::memset(&Sv[0], 0, sizeof(Shared));
        SerialExec ex;
        if (P.form == 1) optimize<1>(ex, obs, P, Sv[0], flags.data(), R);
        else optimize<0>(ex, obs, P, Sv[0], flags.data(), R);
        double sigma[15] = {0}, eigs[15] = {0};
        finish_prior(P.form, R, sigma, eigs);
        std::fwrite(&R, sizeof(R), 1, out);
        if (n) std::fwrite(flags.data(), 1, n, out);
        if (n) std::fwrite(obs.chi2.data(), 8, n, out);
        std::fwrite(sigma, 8, 15, out);
        std::fwrite(eigs, 8, 15, out);
        std::printf("scene %d: form %d n %d bad %d inliers %d rounds %d %d %d %d failed %d %d %d %d\n", sidx, P.form, P.n, R.n_bad, R.n_inliers,
                    R.iterations[0], R.iterations[1], R.iterations[2], R.iterations[3], R.solve_failed[0], R.solve_failed[1],
                    R.solve_failed[2], R.solve_failed[3]);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
