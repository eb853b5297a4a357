// CPU checks of the host-memory admission table (ms-slam_amd/csrc/host_admission.h) and of the pinned pool / cv::MatAllocator
// adaptor (ms-slam_amd/host/PinnedMat.h) with malloc backends: no HIP, no libmsorb.so.  tests/test_host_admission_cpu.py builds
// and runs it, one section per test.   usage: host_admission_main <lookup|holds|threads|pool|adaptor>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

#include "PinnedMat.h"
#include "host_admission.h"

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } \
    } while (0)

namespace {
std::atomic<int> g_allocs{0}, g_frees{0}, g_pins{0}, g_unpins{0};
constexpr unsigned char kLive = 0x11, kDead = 0xdd;
int be_alloc(size_t bytes, void** out) { *out = std::malloc(bytes); std::memset(*out, kLive, bytes < 64 ? bytes : 64); g_allocs++; return *out ? 0 : -3; }
int be_free(void* p) { *static_cast<volatile unsigned char*>(p) = kDead; std::free(p); g_frees++; return 0; }
int be_pin(void*, size_t, int* adopted) { *adopted = 0; g_pins++; return 0; }
int be_unpin(void*) { g_unpins++; return 0; }
const msorb::HostPinBackend kBackend{be_alloc, be_free, be_pin, be_unpin};
using Table = msorb::HostAdmission;

void lookup() {
    Table t(kBackend);
    static unsigned char arena[4096];
    CHECK(!t.admitted(arena, 1) && t.size() == 0);                      // an empty table admits nothing
    CHECK(t.add(arena + 100, 200) == 0 && t.add(arena + 300, 100) == 0);   // [100, 300) and the adjacent [300, 400)
    CHECK(t.add(arena + 1000, 16) == 0);
    CHECK(t.admitted(arena + 100, 200) && t.admitted(arena + 150, 1) && t.admitted(arena + 299, 1) && t.admitted(arena + 300, 100));
    CHECK(!t.admitted(arena + 99, 2) && !t.admitted(arena + 99, 1));    // the first byte outside
    CHECK(!t.admitted(arena + 100, 201) && !t.admitted(arena + 399, 2) && !t.admitted(arena + 400, 1));   // the last byte outside
    CHECK(!t.admitted(arena + 250, 100));                               // spans two adjacent entries: inside no ONE entry
    CHECK(!t.admitted(arena + 500, 10) && !t.admitted(arena + 1016, 1) && !t.admitted(arena, 4096));
    CHECK(!t.admitted(nullptr, 1) && !t.admitted(arena + 100, 0) && !t.admitted(arena + 100, ~(size_t)0));
    CHECK(t.remove(arena + 100) == 0 && !t.admitted(arena + 150, 1) && t.admitted(arena + 300, 1));   // an entry that has left the table
    CHECK(t.remove(arena + 100) == Table::kInvalid && t.size() == 2);
}

void holds() {
    Table t(kBackend);
    static unsigned char arena[4096];
    CHECK(t.add(arena + 1000, 1000) == 0);
    const int pins = g_pins;
    for (auto r : {std::pair<int, int>{500, 501}, {1999, 10}, {1200, 10}, {0, 4096}, {1000, 1000}})
        CHECK(t.add(arena + r.first, (size_t)r.second) == Table::kInvalid);   // overlapping registrations are refused,
    CHECK(g_pins == pins);                                                    // before anything is pinned
    CHECK(t.add(arena + 500, 500) == 0 && t.add(arena + 2000, 1) == 0);       // touching is not overlapping
    void* p = nullptr;
    CHECK(t.alloc(4096, &p) == 0 && p && t.admitted(p, 4096) && !t.admitted(p, 4097));
    CHECK(t.alloc(0, &p) == Table::kInvalid && p == nullptr);
    CHECK(t.alloc(4096, &p) == 0);
    // free / unregister of a held entry free nothing
    Table::Entry* e = t.hold(static_cast<unsigned char*>(p) + 7, 100);
    CHECK(e && e->base == reinterpret_cast<uintptr_t>(p) && e->kind == Table::kAllocated);
    Table::Entry* e2 = t.hold(p, 4096);
    const int frees = g_frees;
    CHECK(e2 == e && t.free(p) == Table::kInvalid && g_frees == frees && t.admitted(p, 1));
    Table::release(e);
    CHECK(t.free(p) == Table::kInvalid);       // still held once
    Table::release(e2);
    CHECK(t.free(p) == 0 && g_frees == frees + 1 && !t.admitted(p, 1) && t.free(p) == Table::kInvalid);
    Table::Entry* r = t.hold(arena + 1500, 10);
    const int unpins = g_unpins;
    CHECK(r && r->kind == Table::kRegistered && t.remove(arena + 1000) == Table::kInvalid && g_unpins == unpins);
    Table::release(r);
    CHECK(t.remove(arena + 1000) == 0 && g_unpins == unpins + 1);
    // the two families do not free each other's entries, and only an entry's first byte names it
    CHECK(t.alloc(64, &p) == 0 && t.remove(p) == Table::kInvalid && t.free(arena + 500) == Table::kInvalid && t.remove(arena + 501) == Table::kInvalid);
    CHECK(t.free(p) == 0 && t.remove(arena + 500) == 0);
    // memory its owner pinned itself is adopted: never unpinned by the table
    msorb::HostPinBackend adopting = kBackend;
    adopting.pin = [](void*, size_t, int* adopted) { *adopted = 1; return 0; };
    Table a(adopting);
    const int unpins2 = g_unpins;
    CHECK(a.add(arena, 64) == 0 && a.admitted(arena, 64) && a.remove(arena) == 0 && g_unpins == unpins2);
    // a backend without a device: nothing enters the table
    msorb::HostPinBackend none{[](size_t, void**) { return -2; }, be_free, [](void*, size_t, int*) { return -2; }, be_unpin};
    Table n(none);
    CHECK(n.alloc(64, &p) == -2 && n.add(arena, 64) == -2 && n.size() == 0);
}

// two lookup threads (the eye threads) against a thread that allocates and frees: a held block is never freed, a stable entry is
// always found, and every block is freed exactly once in the end
void threads() {
    Table t(kBackend);
    void* stable = nullptr;
    CHECK(t.alloc(1 << 16, &stable) == 0);
    std::atomic<void*> slot{nullptr};
    std::atomic<bool> done{false};
    std::atomic<long> hits{0}, refused{0};
    const int a0 = g_allocs, f0 = g_frees;
    constexpr int kIter = 20000;
    auto looker = [&] {
        for (int i = 0; i < kIter || !done; i++) {
            CHECK(t.admitted(static_cast<unsigned char*>(stable) + (i & 0xfff), 64));
            void* p = slot.load();
            if (!p) continue;
            Table::Entry* e = t.hold(p, 64);
            if (!e) continue;   // freed (or freed and not yet replaced) since the load: simply not admitted
            for (int k = 0; k < 8; k++) CHECK(*static_cast<volatile unsigned char*>(p) == kLive);   // held: not freed under us
            hits++;
            Table::release(e);
        }
    };
    std::thread l1(looker), l2(looker);
    for (int i = 0; i < kIter; i++) {
        void* p = nullptr;
        CHECK(t.alloc(256 + (i & 255), &p) == 0);
        slot.store(p);
        if ((i & 15) == 0) std::this_thread::yield();
        slot.store(nullptr);
        while (t.free(p) != 0) refused++;   // refused while a lookup thread holds it, never pulled from under it
    }
    done = true;
    l1.join(); l2.join();
    CHECK(t.free(stable) == 0 && t.size() == 0);
    CHECK(g_allocs - a0 == kIter && g_frees - f0 == kIter + 1);
    std::printf("threads: %ld held lookups, %ld refused frees\n", hits.load(), refused.load());
}

std::atomic<int> g_pool_allocs{0}, g_pool_frees{0};
int pool_alloc(size_t bytes, void** out) { *out = std::malloc(bytes); g_pool_allocs++; return *out ? 0 : -3; }
int pool_free(void* p) { std::free(p); g_pool_frees++; return 0; }

void pool() {
    using msorb_host::PinnedPool;
    {
        PinnedPool p(msorb_host::PinnedBackend{pool_alloc, pool_free});
        void* a = p.acquire(466656);   // a KITTI image: the 512 KB class
        CHECK(a && g_pool_allocs == 1 && p.held_bytes() == (size_t)512 << 10 && p.owns(a));
        CHECK(p.release(a) && !p.release(a) && g_pool_frees == 0 && p.idle_bytes() == (size_t)512 << 10);   // never freed on release
        void* b = p.acquire(300000);   // the same class: the released block, no backend call
        CHECK(b == a && g_pool_allocs == 1);
        void* c = p.acquire(466656);
        CHECK(c && c != a && g_pool_allocs == 2);
        void* d = p.acquire(100);      // another class
        CHECK(d && g_pool_allocs == 3 && p.held_bytes() == ((size_t)1 << 20) + 4096);
        int on_stack;
        CHECK(!p.release(&on_stack) && !p.owns(&on_stack));
        // budget: idle blocks are trimmed, blocks in use never
        CHECK(p.release(c));
        p.set_budget((size_t)600 << 10);
        CHECK(g_pool_frees == 1 && p.idle_bytes() == 0 && p.held_bytes() == ((size_t)512 << 10) + 4096 && p.owns(b) && p.owns(d));
        p.set_budget(4096);            // below what is in use: nothing more can go
        CHECK(g_pool_frees == 1 && p.owns(b) && p.owns(d));
        void* e = p.acquire(466656);   // over budget with nothing idle: served all the same
        CHECK(e && g_pool_allocs == 4);
        CHECK(p.release(e) && g_pool_frees == 2 && p.release(b) && g_pool_frees == 3 && p.release(d) && g_pool_frees == 3);   // d fits the budget: kept
        CHECK(p.idle_bytes() == 4096 && p.held_bytes() == 4096);
        CHECK(p.acquire(~(size_t)0) == nullptr);
    }
    CHECK(g_pool_frees == 4 && g_pool_allocs == 4);   // the pool's destructor returns its idle blocks
}

void adaptor() {
    using namespace msorb_host;
    g_pool_allocs = g_pool_frees = 0;
    PinnedPool p(PinnedBackend{pool_alloc, pool_free});
    PinnedMatAllocator alloc(&p);
    CHECK(alloc.threshold() == 64 * 1024);
    cv::Mat::setDefaultAllocator(&alloc);
    {
        cv::Mat small;
        small.create(3, 3, CV_8UC1);           // below the threshold: the standard allocator, the pool is not asked
        cv::Mat desc;
        desc.create(2000, 32, CV_8U);          // 64 000 bytes: a descriptor Mat stays pageable too
        CHECK(g_pool_allocs == 0 && p.held_bytes() == 0 && !p.owns(small.data) && !p.owns(desc.data));
        small.data[8] = 1;
        unsigned char user[256 * 512];
        cv::Mat over_user(256, 512, CV_8UC1, user, 512);   // a Mat over the application's memory allocates nothing
        CHECK(g_pool_allocs == 0);
        cv::Mat im;
        im.create(376, 1241, CV_8UC1);
        CHECK(g_pool_allocs == 1 && p.owns(im.data) && im.step == 1241 && im.rows == 376 && im.cols == 1241);
        for (int y = 0; y < im.rows; y++) std::memset(im.ptr<unsigned char>(y), y & 255, (size_t)im.cols);
        cv::Mat c = im.clone();                // System.cc:215-216
        CHECK(g_pool_allocs == 2 && p.owns(c.data) && c.data != im.data && c.ptr<unsigned char>(375)[1240] == (375 & 255));
        cv::Mat share = c;                     // a copy shares the block; the last owner gives it back
        unsigned char* const cdata = c.data;
        c.release();
        CHECK(p.owns(cdata) && share.data == cdata);
        share.release();
        CHECK(!p.owns(cdata) && p.idle_bytes() == (size_t)512 << 10 && g_pool_frees == 0);
        cv::Mat next = im.clone();             // the next frame: the released block again, no backend call
        CHECK(next.data == cdata && g_pool_allocs == 2);
    }
    CHECK(p.idle_bytes() == (size_t)1 << 20 && g_pool_frees == 0);
    cv::Mat::setDefaultAllocator(cv::Mat::getStdAllocator());
}
}  // namespace

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "all";
    bool any = false;
    const struct { const char* name; void (*fn)(); } sections[] = {{"lookup", lookup}, {"holds", holds}, {"threads", threads}, {"pool", pool}, {"adaptor", adaptor}};
    for (const auto& s : sections)
        if (what == "all" || what == s.name) { s.fn(); std::printf("ok %s\n", s.name); any = true; }
    return any ? 0 : 2;
}
