// TEST-ONLY stand-in for DUtils::Random of the reference's Thirdparty/DBoW2 (same class and method names) for
// tests/dropin_two_view_main.cc: SeedRandOnce(seed) seeds the C library's rand() once per process, as the reference's does, and
// RandomInt is the reference's expression over rand(); both are counted, so that the test sees how rand() was consumed.
#pragma once
#include <cstdlib>

namespace DUtils {
class Random {
public:
    static int& Seedings() { static int n = 0; return n; }     // calls of SeedRandOnce that seeded
    static int& LastSeed() { static int s = -1; return s; }
    static long& Draws() { static long n = 0; return n; }      // calls of RandomInt
    static void SeedRandOnce(int seed) {
        static bool already_seeded = false;
        if (!already_seeded) {
            std::srand((unsigned)seed);
            already_seeded = true;
            Seedings()++;
            LastSeed() = seed;
        }
    }
    static int RandomInt(int min, int max) {
        Draws()++;
        const int d = max - min + 1;
        return (int)(((double)std::rand() / ((double)RAND_MAX + 1.0)) * d) + min;
    }
};
}  // namespace DUtils
