// TwoViewReconstruction::Reconstruct over ALL hypotheses on the host: ms-slam_amd/csrc/two_view_device.h and two_view_select.h
// compiled for the host (-O2 -ffp-contract=off, no SIMD intrinsics) through tests/two_view_host_path.h, on one thread and on the
// reference's two (FindHomography and FindFundamental side by side, :105-110).  The yardstick of tools/two_view_latency.py.
//   two_view_host <scenes.bin> <reps>        one scene in the format of tests/two_view_cases.py (write_scenes)
//   prints: median_ms(1 thread) min_ms(1) median_ms(2 threads) min_ms(2) ok branch winner_h winner_f chosen sum_of_counts
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../tests/two_view_host_path.h"

template <class T> static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) std::exit(2);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || take<int>(f, 1)[0] != 1) return 2;
    const std::vector<int> hd = take<int>(f, 4);
    const std::vector<float> fl = take<float>(f, 6);
    tv_host::Problem p;
    p.n1 = hd[0]; p.n2 = hd[1]; p.n_hyp = hd[2]; p.min_triangulated = hd[3];
    for (int k = 0; k < 4; k++) p.cam[k] = fl[k];
    p.sigma = fl[4]; p.min_parallax = fl[5];
    p.h_ratio = take<double>(f, 1)[0];
    p.keys1 = take<float>(f, 2 * (size_t)p.n1);
    p.keys2 = take<float>(f, 2 * (size_t)p.n2);
    p.matches12 = take<int>(f, p.n1);
    p.sets = take<int>(f, 8 * (size_t)p.n_hyp);
    std::fclose(f);
    const int reps = std::atoi(argv[2]);
    double med[2], mn[2];
    tv_host::Answer a;
    for (int threads = 1; threads <= 2; threads++) {
        std::vector<double> ms;
        for (int rep = 0; rep < reps; rep++) {
            const auto t0 = std::chrono::steady_clock::now();
            a = tv_host::reconstruct(p, threads);
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        med[threads - 1] = ms[ms.size() / 2];
        mn[threads - 1] = ms[0];
    }
    long long sum = 0;
    for (int c : a.counts) sum += c;
    std::printf("%.6f %.6f %.6f %.6f %d %d %d %d %d %lld\n", med[0], mn[0], med[1], mn[1], a.r.ok, a.r.branch, a.r.winner_h, a.r.winner_f, a.r.chosen, sum);
    return 0;
}
