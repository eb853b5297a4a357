// The per-thread scratch protocol of ms-slam_amd/csrc/hip_host.h (ThreadScratch, DevBuf, PinBuf) against the HIP stand-in of
// tests/hip_stub, on the CPU: the stub aborts when an object is destroyed or freed with another device current than the one it was
// created on, and records every creation, so the checks below see on which device each object was made and in which order.
// Prints one line per failed check to stderr and "ok" on stdout when every check held.
// usage: thread_scratch
#include <cstdio>
#include <string>
#include <thread>

#include "hip_host.h"

namespace msorb {
static std::string g_error;
void set_last_error(const std::string& s) { g_error = s; }
}  // namespace msorb

using hip_stub::state;
using msorb::DevBuf;
using msorb::PinBuf;
using msorb::ThreadScratch;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                            \
        }                                                                        \
    } while (0)

static size_t count(const std::vector<hip_stub::Object>& v, size_t from, char kind, int device) {
    size_t n = 0;
    for (size_t i = from; i < v.size(); i++) n += v[i].kind == kind && v[i].device == device;
    return n;
}

static void switch_device() {
    ThreadScratch s(true, 2);
    CHECK(s.acquire(0, 100, 40) == MSORB_OK);
    CHECK(s.device == 0 && state().current == 0);
    CHECK(s.s && s.ev[0] && s.ev[1] && s.d.p && s.h.p);
    const size_t c0 = state().created.size(), d0 = state().destroyed.size();
    CHECK(hipSetDevice(1) == hipSuccess);   // the caller has moved on to device 1 already
    CHECK(s.acquire(1, 100, 40) == MSORB_OK);
    // device 0's stream, events and blocks were destroyed (the stub aborts on a wrong current device) ...
    CHECK(state().destroyed.size() - d0 == 5);
    CHECK(count(state().destroyed, d0, 's', 0) == 1 && count(state().destroyed, d0, 'e', 0) == 2);
    CHECK(count(state().destroyed, d0, 'd', 0) == 1 && count(state().destroyed, d0, 'h', 0) == 1);
    // ... and device 1's were created while device 1 was current
    CHECK(state().created.size() - c0 == 5);
    CHECK(count(state().created, c0, 's', 1) == 1 && count(state().created, c0, 'e', 1) == 2);
    CHECK(count(state().created, c0, 'd', 1) == 1 && count(state().created, c0, 'h', 1) == 1);
    CHECK(state().live.at(s.s).device == 1 && state().live.at(s.d.p).device == 1 && state().live.at(s.h.p).device == 1);
    CHECK(s.device == 1 && state().current == 1);

    // the same device again: nothing is created or freed while the blocks are large enough (1.5x headroom)
    const size_t c1 = state().created.size(), d1 = state().destroyed.size();
    CHECK(s.acquire(1, 100, 40) == MSORB_OK);
    CHECK(s.acquire(1, 150, 60) == MSORB_OK);
    CHECK(state().created.size() == c1 && state().destroyed.size() == d1);
    // past its capacity a block grows, alone
    CHECK(s.acquire(1, 151, 60) == MSORB_OK);
    CHECK(state().created.size() == c1 + 1 && state().destroyed.size() == d1 + 1);
    CHECK(state().created.back().kind == 'd' && state().created.back().device == 1 && state().created.back().bytes == 151 + 75 + 16);
    CHECK(s.d.n == 151 + 75);
    CHECK(hipSetDevice(0) == hipSuccess);
    s.release();   // frees on device 1
    CHECK(s.device == -1 && !s.s && !s.d.p && !s.h.p);
}

static void failed_creation() {
    ThreadScratch s(true, 2);
    msorb::g_error.clear();
    const size_t live0 = state().live.size();
    state().fail_stream_on = 1;
    CHECK(s.acquire(1, 64, 64) == MSORB_E_HIP);
    state().fail_stream_on = -1;
    CHECK(!msorb::g_error.empty());
    CHECK(s.device == -1 && !s.s && !s.ev[0] && !s.ev[1] && !s.d.p && !s.h.p);
    CHECK(state().live.size() == live0);
    const size_t c0 = state().created.size();
    CHECK(s.acquire(1, 64, 64) == MSORB_OK);   // the next call starts clean
    CHECK(s.device == 1 && s.s && count(state().created, c0, 's', 1) == 1);

    // a failure after the stream and the events exist releases them on the device they were made on
    ThreadScratch t(true, 2);
    const size_t d0 = state().destroyed.size();
    CHECK(hipSetDevice(1) == hipSuccess);
    state().fail_malloc_on = 0;
    CHECK(t.acquire(0, 64, 64) == MSORB_E_HIP);
    state().fail_malloc_on = -1;
    CHECK(t.device == -1 && !t.s && !t.ev[0] && !t.ev[1]);
    CHECK(count(state().destroyed, d0, 's', 0) == 1 && count(state().destroyed, d0, 'e', 0) == 2);
    CHECK(state().live.size() == live0 + 5);   // only s's objects
    CHECK(state().current == 0);
}

static void no_stream() {
    ThreadScratch s(false, 2);
    const size_t c0 = state().created.size();
    CHECK(s.acquire(0, 32, 0) == MSORB_OK);
    CHECK(!s.s && s.ev[0] && s.ev[1] && !s.ev[2]);
    CHECK(count(state().created, c0, 's', 0) == 0 && count(state().created, c0, 'e', 0) == 2);
    CHECK(count(state().created, c0, 'd', 0) == 1 && count(state().created, c0, 'h', 0) == 0);
    ThreadScratch b(false, 0);   // a device block only
    const size_t c1 = state().created.size();
    CHECK(b.acquire(0, 32, 0) == MSORB_OK);
    CHECK(!b.s && !b.ev[0] && state().created.size() == c1 + 1);
}

static void thread_exit() {
    auto body = [](int dev) {
        static thread_local ThreadScratch s(true, 2);
        CHECK(s.acquire(dev, 64, 64) == MSORB_OK);
    };
    // a live runtime: the thread's objects are freed at its exit, with their device current (else the stub aborts)
    size_t d0 = state().destroyed.size();
    std::thread([&] { body(1); hipSetDevice(0); }).join();
    CHECK(count(state().destroyed, d0, 's', 1) == 1 && count(state().destroyed, d0, 'e', 1) == 2);
    CHECK(count(state().destroyed, d0, 'd', 1) == 1 && count(state().destroyed, d0, 'h', 1) == 1);
    // a runtime that has shut down (hipSetDevice fails): nothing is freed
    const size_t live0 = state().live.size();
    d0 = state().destroyed.size();
    std::thread([&] { body(1); hipSetDevice(0); state().fail_set_device = true; }).join();
    state().fail_set_device = false;
    CHECK(state().destroyed.size() == d0);
    CHECK(state().live.size() == live0 + 5);
}

static void buffers() {
    DevBuf<int> d;
    PinBuf<double> h;
    const size_t c0 = state().created.size();
    CHECK(d.ensure(0) == MSORB_OK && h.ensure(0) == MSORB_OK);
    CHECK(state().created.size() == c0 && !d.p && !h.p);
    CHECK(d.ensure(10) == MSORB_OK && h.ensure(3) == MSORB_OK);
    CHECK(state().created.size() == c0 + 2);
    CHECK(state().created[c0].kind == 'd' && state().created[c0].bytes == 10 * sizeof(int) + 16);
    CHECK(state().created[c0 + 1].kind == 'h' && state().created[c0 + 1].bytes == 3 * sizeof(double) + 16);
    CHECK(d.ensure(10) == MSORB_OK && d.ensure(4) == MSORB_OK && state().created.size() == c0 + 2);   // grow-only
    CHECK(d.ensure(11) == MSORB_OK && state().created.size() == c0 + 3 && state().created.back().bytes == 11 * sizeof(int) + 16);
    d.release();
    h.release();
    CHECK(!d.p && d.n == 0 && !h.p && h.n == 0);
}

int main() {
    CHECK(msorb::require_device(1) == MSORB_OK);
    CHECK(msorb::require_device(2) == MSORB_E_NO_DEVICE && msorb::require_device(-1) == MSORB_E_NO_DEVICE);
    CHECK(msorb::up16(0) == 0 && msorb::up16(1) == 16 && msorb::up16(16) == 16 && msorb::up16(17) == 32);
    switch_device();
    failed_creation();
    no_stream();
    thread_exit();
    buffers();
    if (g_fail) return 1;
    std::printf("ok\n");
    return 0;
}
