// ms-slam_amd/csrc/new_points_device.h on the CPU (tests/test_new_map_points_cpu.py): the per-pair arithmetic of
// LocalMapping::CreateNewMapPoints over the pairs of a file, compiled with g++ -ffp-contract=off, plain and under the sanitizers.
//   in : int32 m, int32 inertial, float th_far, float ratio_factor, NpCam c1, NpCam c2 (23 floats each), m x (NpFeature f1, NpFeature f2)
//   out: m status bytes, then m x 3 floats
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ms-slam_amd/csrc/new_points_device.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t m = 0, inertial = 0;
    float th_far = 0, ratio_factor = 0;
    msorb::NpCam c1, c2;
    static_assert(sizeof(msorb::NpCam) == 23 * 4 && sizeof(msorb::NpFeature) == 6 * 4, "file layout");
    bool ok = fread(&m, 4, 1, in) == 1 && fread(&inertial, 4, 1, in) == 1 && fread(&th_far, 4, 1, in) == 1 &&
              fread(&ratio_factor, 4, 1, in) == 1 && fread(&c1, sizeof(c1), 1, in) == 1 && fread(&c2, sizeof(c2), 1, in) == 1 && m >= 0;
    std::vector<msorb::NpFeature> f(ok ? 2 * (size_t)m : 0);
    ok = ok && fread(f.data(), sizeof(msorb::NpFeature), f.size(), in) == f.size();
    fclose(in);
    if (!ok) return 3;
    std::vector<uint8_t> status((size_t)m);
    std::vector<float> x((size_t)m * 3, 0.0f);
    for (int i = 0; i < m; i++) {
        float X[3] = {0, 0, 0};
        status[i] = msorb::new_point_pair(c1, c2, f[2 * (size_t)i], f[2 * (size_t)i + 1], inertial, th_far, ratio_factor, X);
        if (status[i] >= msorb::kNpTriangulated && status[i] <= msorb::kNpStereo2)
            for (int k = 0; k < 3; k++) x[3 * (size_t)i + k] = X[k];
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    ok = fwrite(status.data(), 1, status.size(), out) == status.size() && fwrite(x.data(), 4, x.size(), out) == x.size();
    return fclose(out) == 0 && ok ? 0 : 3;
}
