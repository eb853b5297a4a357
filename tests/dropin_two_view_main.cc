// msorb_host::TwoViewReconstruction (ms-slam_amd/host/TwoViewReconstruction_device.h) over the stand-ins of tests/slam_stub and
// tests/cv_stub, driven as Pinhole::ReconstructWithTwoViews drives the reference's class (Pinhole.cpp:83-91).
//   dropin_two_view <scene.bin> <out.bin>      one scene in the format of tests/two_view_cases.py (write_scenes); its sets are ignored:
//                                              the class draws its own
// out: int32 returned, seedings, last seed; int64 draws; T21 (R 9 floats, t 3); vbTriangulated [n1] u8; vP3D [n1 x 3]; the
// winner's points [n1 x 3] (zeros when empty); int32 branch; then the same return value and draws of a second Reconstruct.
// vP3D and vbTriangulated enter filled with 7 / true and T21 as the identity, so that what the class leaves alone shows.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sim3_stub_types.h"
#include "TwoViewReconstruction_device.h"

namespace {
struct Point3 { float x, y, z; };
typedef ORB_SLAM3::msorb_host::TwoViewReconstruction<cv::KeyPoint, Point3, Sophus::SE3f, sim3_stub::Matrix3f, sim3_stub::Vector3f> Tvr;

template <class T> std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return v;
}
template <class T> void put(FILE* f, const T* p, size_t n) { if (n) std::fwrite(p, sizeof(T), n, f); }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: dropin_two_view <scene.bin> <out.bin>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    if (take<int>(f, 1)[0] != 1) return 2;
    const std::vector<int> hd = take<int>(f, 4);
    const std::vector<float> fl = take<float>(f, 6);
    take<double>(f, 1);
    const int n1 = hd[0], n2 = hd[1], H = hd[2];
    const std::vector<float> k1 = take<float>(f, 2 * (size_t)n1), k2 = take<float>(f, 2 * (size_t)n2);
    const std::vector<int> m12 = take<int>(f, n1);
    std::fclose(f);
    std::vector<cv::KeyPoint> keys1(n1), keys2(n2);
    for (int i = 0; i < n1; i++) { keys1[i] = cv::KeyPoint{}; keys1[i].pt.x = k1[2 * (size_t)i]; keys1[i].pt.y = k1[2 * (size_t)i + 1]; }
    for (int i = 0; i < n2; i++) { keys2[i] = cv::KeyPoint{}; keys2[i].pt.x = k2[2 * (size_t)i]; keys2[i].pt.y = k2[2 * (size_t)i + 1]; }
    const Eigen::Matrix3f K{{fl[0], 0, fl[2], 0, fl[1], fl[3], 0, 0, 1}};
    Tvr tvr(K, fl[4], H);
    Sophus::SE3f T21;
    std::vector<Point3> vP3D(n1, Point3{7, 7, 7});
    std::vector<bool> vbTriangulated(n1, true);
    const int ok = tvr.Reconstruct(keys1, keys2, m12, T21, vP3D, vbTriangulated);
    const int head[3] = {ok, DUtils::Random::Seedings(), DUtils::Random::LastSeed()};
    const long long draws = DUtils::Random::Draws();
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    put(o, head, 3);
    put(o, &draws, 1);
    put(o, T21.R.m, 9);
    put(o, T21.t.v, 3);
    std::vector<uint8_t> tri(n1);
    for (int i = 0; i < n1; i++) tri[i] = vbTriangulated[i];
    put(o, tri.data(), tri.size());
    put(o, reinterpret_cast<const float*>(vP3D.data()), 3 * (size_t)n1);
    std::vector<Point3> w = tvr.GetWinnerPoints();
    w.resize(n1, Point3{0, 0, 0});
    put(o, reinterpret_cast<const float*>(w.data()), 3 * (size_t)n1);
    const int branch = tvr.GetBranch();
    put(o, &branch, 1);
    // a second Reconstruct: SeedRandOnce does not seed again, and another 8 * iterations draws are taken
    const int ok2 = tvr.Reconstruct(keys1, keys2, m12, T21, vP3D, vbTriangulated);
    const int tail[2] = {ok2, DUtils::Random::Seedings()};
    const long long draws2 = DUtils::Random::Draws();
    put(o, tail, 2);
    put(o, &draws2, 1);
    std::fclose(o);
    return 0;
}
