// The loop of Sim3Solver::iterate over ALL hypotheses on one host core: ms-slam_amd/csrc/sim3_device.h and sim3_select.h compiled
// for the host (-O2 -ffp-contract=off), one thread, no SIMD intrinsics.  The yardstick of tools/sim3_ransac_latency.py.
//   sim3_ransac_host <scene.bin> <reps>
//   scene: int32 n, H, fix_scale, min_inliers, best_in; float cam1[4], cam2[4], X1[3 n], X2[3 n], max_err1[n], max_err2[n];
//          int32 triples[3 H]
//   prints: median_ms min_ms winner converged consumed sum_of_counts
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sim3_device.h"
#include "sim3_select.h"

template <class T> static bool rd(FILE* f, T* p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t hdr[5];
    float cam1[4], cam2[4];
    if (!rd(in, hdr, 5) || !rd(in, cam1, 4) || !rd(in, cam2, 4) || hdr[0] < 3 || hdr[1] < 1) return 2;
    const int n = hdr[0], H = hdr[1], reps = std::atoi(argv[2]);
    std::vector<float> X1(3 * (size_t)n), X2(3 * (size_t)n), e1(n), e2(n);
    std::vector<int32_t> tr(3 * (size_t)H);
    if (!rd(in, X1.data(), X1.size()) || !rd(in, X2.data(), X2.size()) || !rd(in, e1.data(), n) || !rd(in, e2.data(), n) || !rd(in, tr.data(), tr.size()))
        return 2;
    std::fclose(in);
    std::vector<int> counts(H);
    std::vector<uint8_t> mask((size_t)H * n);
    std::vector<double> ms;
    msorb::Sim3Selection sel{};
    for (int rep = 0; rep < reps; rep++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int h = 0; h < H; h++) {
            float P1[9], P2[9];
            for (int i = 0; i < 3; i++) {
                std::memcpy(P1 + 3 * i, &X1[3 * (size_t)tr[3 * (size_t)h + i]], 12);
                std::memcpy(P2 + 3 * i, &X2[3 * (size_t)tr[3 * (size_t)h + i]], 12);
            }
            msorb::Sim3Transform T;
            msorb::sim3_compute(P1, P2, hdr[2] != 0, T);
            int c = 0;
            uint8_t* m = &mask[(size_t)h * n];
            for (int i = 0; i < n; i++) {
                m[i] = msorb::sim3_is_inlier(T, cam1, cam2, &X1[3 * (size_t)i], &X2[3 * (size_t)i], e1[i], e2[i]);
                c += m[i];
            }
            counts[h] = c;
        }
        sel = msorb::sim3_select(counts.data(), H, hdr[3], hdr[4]);
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    long long sum = 0;
    for (int c : counts) sum += c;
    std::printf("%.6f %.6f %d %d %d %lld\n", ms[ms.size() / 2], ms[0], sel.winner, sel.converged, sel.consumed, sum);
    return 0;
}
