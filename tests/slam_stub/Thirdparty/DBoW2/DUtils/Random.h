// TEST-ONLY stand-in for DUtils::Random of the reference's Thirdparty/DBoW2 (same class and method names): uniform integers over
// the C library's rand(), so that a test can feed a Python restatement the same sequence through srand / rand.
#pragma once
#include <cstdlib>

namespace DUtils {
class Random {
public:
    static void SeedRand(int seed) { std::srand((unsigned)seed); }
    // an integer in [min, max]: rand() scaled to [0, 1) in double, times the width, truncated
    static int RandomInt(int min, int max) {
        const double unit = (double)std::rand() / ((double)RAND_MAX + 1.0);
        return (int)(unit * (max - min + 1)) + min;
    }
};
}  // namespace DUtils
