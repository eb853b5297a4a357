// ms-slam_amd/csrc/inertial_device.h (the text the kernel compiles) and inertial_plan.h on the host, serially: one executor walks
// every edge and row in ascending order, every sum is added left to right, the cyclic reduction runs its levels one row after the
// other.
//
//   inertial_opt_main in.bin out.bin        the scenes of tests/inertial_opt_cases.py's write_scenes -> read_results
//   inertial_opt_main --plans in.bin        structures for make_plan alone: prints one PlanError per line
// The last column of a scene's printed line is the wall time of the optimisation alone, which tools/inertial_optimization_latency.py
// reads.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../ms-slam_amd/csrc/inertial_device.h"
#include "../ms-slam_amd/csrc/inertial_plan.h"

using namespace msorb::inertial;

namespace {

struct SerialExec {
    int tid() const { return 0; }
    int stride() const { return 1; }
    void barrier() {}
    void sum(double*, int) {}
    double max1(double v) { return v; }
};

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

int plans(const char* path) {
    FILE* in = std::fopen(path, "rb");
    int n = 0;
    if (!in || !read_exact(in, &n, 4)) return 2;
    for (int i = 0; i < n; i++) {
        int dims[2];
        if (!read_exact(in, dims, 8) || dims[1] < 0) return 2;
        std::vector<int> prev((size_t)dims[1]), cur((size_t)dims[1]);
        if (!read_exact(in, prev.data(), prev.size() * 4) || !read_exact(in, cur.data(), cur.size() * 4)) return 2;
        Plan plan;
        const PlanError pe = make_plan(dims[0], dims[1], prev.data(), cur.data(), plan);
        std::printf("%d %zu\n", (int)pe, plan.row_kf.size());
    }
    std::fclose(in);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "--plans")) return plans(argv[2]);
    if (argc < 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int n_scenes = 0;
    if (!read_exact(in, &n_scenes, 4)) return 2;
    for (int sidx = 0; sidx < n_scenes; sidx++) {
        int dims[2];
        if (!read_exact(in, dims, 8)) return 2;
        const int nk = dims[0], ne = dims[1];
        msorb_inertial_problem P;
        std::vector<msorb_inertial_keyframe> kfs((size_t)nk);
        std::vector<msorb_inertial_edge> edges((size_t)ne);
        if (!read_exact(in, &P, sizeof(P)) || !read_exact(in, kfs.data(), kfs.size() * sizeof(kfs[0])) ||
            !read_exact(in, edges.data(), edges.size() * sizeof(edges[0])))
            return 2;
        std::vector<int> prev((size_t)ne), cur((size_t)ne);
        for (int e = 0; e < ne; e++) { prev[e] = edges[e].kf_prev; cur[e] = edges[e].kf_cur; }
        Plan plan;
        if (make_plan(nk, ne, prev.data(), cur.data(), plan) != kPlanOk) return 3;
        const size_t nr = plan.row_kf.size();
        std::vector<double> v(6 * (size_t)nk + 1), W((size_t)kEdgeW * ne + 1), chi2((size_t)ne + 1), D(9 * nr + 1), L(9 * nr + 1), U(9 * nr + 1),
            R(3 * kRhs * nr + 1), R0(3 * kRhs * nr + 1), x(3 * nr + 1);
        Work K{nk, ne, (int)nr, kfs.data(), edges.data(), plan.row_kf.data(), plan.e_prev.data(), plan.e_next.data(), v.data(), W.data(),
               chi2.data(), D.data(), L.data(), U.data(), R.data(), R0.data(), x.data()};
        msorb_inertial_result res;
        std::memset(&res, 0, sizeof(res));
        SerialExec ex;
        const auto t0 = std::chrono::steady_clock::now();
        optimize(ex, K, P, res);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::fwrite(&res, sizeof(res), 1, out);
        std::fwrite(v.data(), 8, 3 * (size_t)nk, out);
        std::fwrite(chi2.data(), 8, (size_t)ne, out);
        std::printf("scene %d: KeyFrames %d edges %d rows %zu status %d iterations %d rejected %d chi2 %.6e -> %.6e ms %.3f\n", sidx, nk, ne, nr,
                    res.status, res.iterations, res.rejected_trials, res.chi2_initial, res.chi2_final, ms);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
