// TEST-ONLY stand-in for DUtils::Random of the reference's Thirdparty/DBoW2 (same class and method names) for
// tests/dropin_mlpnp_main.cc: a 64-bit linear congruential generator of its own, which tests/test_dropin_mlpnp_gpu.py restates, so
// that the draws of the test depend on nothing else in the process (the stand-in of tests/slam_stub draws from the C library's
// rand(), which the process shares).
#pragma once
#include <cstdint>

namespace DUtils {
class Random {
public:
    static inline uint64_t state = 0;
    static void SeedRand(int seed) { state = (uint64_t)(uint32_t)seed; }
    // an integer in [min, max]: the top 31 bits of the next state scaled to [0, 1) in double, times the width, truncated
    static int RandomInt(int min, int max) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        const double unit = (double)(state >> 33) / 2147483648.0;
        return (int)(unit * (max - min + 1)) + min;
    }
};
}  // namespace DUtils
