// How far the float arctangent of ms-slam_amd/csrc/pose_rig_device.h (a double atan2 of the widened arguments, narrowed once) is from
// the installed libm's atan2f, which KannalaBrandt8::project(Vector3d) calls (KannalaBrandt8.cpp:48-49), over the (y, x) that
// projection sees: theta = atan2f(sqrtf(x^2 + y^2), z) and psi = atan2f(y, x) of camera-frame points 0.3 - 50 m away, theta from
// 1e-3 to 100 degrees (z < 0 beyond 90), psi over the whole circle.  Prints one JSON line: per use the number of inputs, the share
// on which the two floats differ and the largest difference in ulp.  No GPU.
//   g++ -std=c++17 -O2 -ffp-contract=off tools/atan2f_departure.cc -o atan2f_departure && ./atan2f_departure [samples]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../ms-slam_amd/csrc/pose_rig_device.h"

namespace {

struct Tally { long n = 0, differ = 0; int max_ulp = 0; };

int ulp_distance(float a, float b) {
    int32_t ia, ib;
    std::memcpy(&ia, &a, 4);
    std::memcpy(&ib, &b, 4);
    if (ia < 0) ia = INT32_MIN - ia;   // order the bit patterns like the values
    if (ib < 0) ib = INT32_MIN - ib;
    const int64_t d = (int64_t)ia - (int64_t)ib;
    return (int)(d < 0 ? -d : d);
}

void compare(Tally& t, float y, float x) {
    const int d = ulp_distance(atan2f(y, x), msorb::rig::atan2f_narrowed(y, x));
    t.n++;
    t.differ += d != 0;
    if (d > t.max_ulp) t.max_ulp = d;
}

double uniform(uint64_t& s) {   // splitmix64
    s += 0x9e3779b97f4a7c15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (double)((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

}  // namespace

int main(int argc, char** argv) {
    const long samples = argc > 1 ? std::atol(argv[1]) : 20000000;
    const double pi = 3.14159265358979323846;
    Tally theta, psi;
    uint64_t seed = 1;
    for (long i = 0; i < samples; i++) {
        const double th = std::exp(std::log(1e-3) + uniform(seed) * (std::log(100.0) - std::log(1e-3))) * pi / 180;   // log-uniform in degrees
        const double ps = (2 * uniform(seed) - 1) * pi;
        const double d = std::exp(std::log(0.3) + uniform(seed) * (std::log(50.0) - std::log(0.3)));
        const double x = std::sin(th) * std::cos(ps) * d, y = std::sin(th) * std::sin(ps) * d, z = std::cos(th) * d;
        compare(theta, msorb::rig::sqrtf_cr((float)(x * x + y * y)), (float)z);
        compare(psi, (float)y, (float)x);
    }
    std::printf("{\"samples\": %ld, \"theta\": {\"share_differ\": %.6g, \"max_ulp\": %d}, \"psi\": {\"share_differ\": %.6g, \"max_ulp\": %d}}\n", samples,
                (double)theta.differ / theta.n, theta.max_ulp, (double)psi.differ / psi.n, psi.max_ulp);
    return 0;
}
