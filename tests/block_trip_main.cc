// BlockLayout and round_trip of ms-slam_amd/csrc/block_trip.h against the HIP stand-in of tests/hip_stub, on the CPU: the offsets of
// the regions, the order of the stream operations ([upload | fill with 0xFF | launch | download | synchronise], the events only when
// a time is asked for), what a trip moves, and that a failed launch is reported under the caller's name, queues nothing behind it
// and releases the scratch.  The stream operations the stand-in does not have are defined here; each appends a letter to g_ops.
// Prints one line per failed check to stderr and "ok" on stdout when every check held.
#include <cstdio>
#include <cstring>
#include <string>

#include <hip/hip_runtime.h>

static std::string g_ops;
static hipError_t g_launch_error = hipSuccess;   // what the next hipGetLastError returns
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
inline hipError_t hipMemsetAsync(void* p, int value, size_t bytes, hipStream_t) { g_ops += 'm'; std::memset(p, value, bytes); return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { g_ops += 'e'; return hipSuccess; }
inline hipError_t hipGetLastError() { g_ops += 'g'; const hipError_t e = g_launch_error; g_launch_error = hipSuccess; return e; }
inline hipError_t hipStreamSynchronize(hipStream_t) { g_ops += 's'; return hipSuccess; }
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { g_ops += 't'; *ms = 0.25f; return hipSuccess; }

#include "block_trip.h"

namespace msorb {
static std::string g_error;
void set_last_error(const std::string& s) { g_error = s; }
hipError_t small_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    g_ops += kind == hipMemcpyHostToDevice ? 'u' : 'd';
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
}  // namespace msorb

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); g_fail = 1; } \
    } while (0)

int main() {
    msorb::ThreadScratch s(true, 2);
    msorb::BlockLayout L;
    const size_t o_a = L.take(5), o_b = L.take(32), o_c = L.take(0);
    L.outputs_begin();
    const size_t o_m = L.take(12), o_n = L.take(4);
    CHECK(o_a == 0 && o_b == 16 && o_c == 48 && L.in_bytes == 48 && o_m == 48 && o_n == 64 && L.end == 80);
    CHECK(s.acquire(0, L.end, L.end) == MSORB_OK);
    std::memset(s.h.p, 3, L.end);
    std::memset(s.d.p, 9, L.end);
    const msorb::BlockTrip trip{s.d.p, s.h.p, L.in_bytes, s.d.p + o_m, 12, s.h.p + o_m, s.d.p + o_m, L.end - o_m};
    float ms = -1.0f;
    CHECK(msorb::round_trip(s, "trip", trip, &ms, [&](hipStream_t st) { CHECK(st == s.s); g_ops += 'L'; s.d.p[o_n] = 42; }) == MSORB_OK);
    CHECK(g_ops == "umeLgedst" && ms == 0.25f);
    CHECK(s.d.p[0] == 3 && s.d.p[47] == 3);                                         // the inputs went up
    CHECK(s.h.p[o_m] == 0xFF && s.h.p[o_m + 11] == 0xFF && s.h.p[o_m + 12] == 9);   // 12 bytes filled, the rest of the region as it was
    CHECK(s.h.p[o_n] == 42 && s.h.p[0] == 3);
    g_ops.clear();
    const msorb::BlockTrip bare{s.d.p, s.h.p, 16, nullptr, 0, s.h.p + o_n, s.d.p + o_n, 4};
    CHECK(msorb::round_trip(s, "trip", bare, nullptr, [&](hipStream_t) { g_ops += 'L'; }) == MSORB_OK);
    CHECK(g_ops == "uLgds");                                                        // no fill, no events
    g_ops.clear();
    g_launch_error = hipErrorOutOfMemory;
    CHECK(msorb::round_trip(s, "my_entry", trip, &ms, [&](hipStream_t) { g_ops += 'L'; }) == MSORB_E_HIP);
    CHECK(g_ops == "umeLg");                                                        // nothing is queued behind a failed launch
    CHECK(msorb::g_error.rfind("my_entry: ", 0) == 0);
    CHECK(s.device == -1 && !s.s && !s.d.p && !s.h.p);                              // released: the next call starts clean
    CHECK(s.acquire(0, 16, 16) == MSORB_OK);
    s.release();
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}
