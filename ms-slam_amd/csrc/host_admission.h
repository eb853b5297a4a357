// The host-memory admission table behind msorb_host_alloc / _free / _register / _unregister / _admitted (include/msorb.h): the
// ONLY source of host addresses a kernel of this library may dereference.  A frame entry looks an image's byte range up here;
// a range wholly inside one entry is read in place by the upload kernel, anything else is staged as before.
//
// Self-contained (no HIP, no other header of the library): the calls that pin and unpin memory are a table of function
// pointers, so the logic runs on a CPU with a malloc backend (tests/host_admission_main.cc).
//
//   - entries are disjoint intervals in a vector sorted by base address; a lookup is a binary search under the shared side
//     of a reader / writer lock (two eye threads look up per frame while a third allocates and frees);
//   - hold() takes a use count on the entry it finds, release() drops it: remove() of a held entry is refused, so pages are never
//     unpinned under a running kernel.  An Entry lives on the heap and is deleted only by the remove() that found it unheld under
//     the exclusive lock, hence a held pointer stays valid without any lock;
//   - nothing is remembered by raw pointer outside the table: an address that was freed and handed out again as pageable memory
//     is simply not found.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <shared_mutex>
#include <vector>

namespace msorb {

struct HostPinBackend {
    int (*alloc)(size_t bytes, void** out);            // pinned allocation; 0 or a negative MSORB_E_* code
    int (*free_)(void* p);
    int (*pin)(void* p, size_t bytes, int* adopted);   // pins pageable memory; *adopted = 1: it was pinned already, by its owner
    int (*unpin)(void* p);                             // (never called for adopted memory)
};

class HostAdmission {
  public:
    static constexpr int kOk = 0, kInvalid = -1;   // MSORB_OK / MSORB_E_INVALID
    static constexpr int kMaxDevices = 16;
    enum Kind { kAllocated, kRegistered, kAdopted };
    struct Entry {
        uintptr_t base = 0, end = 0;   // [base, end)
        Kind kind = kAllocated;
        std::atomic<int> uses{0};
        // what hipHostGetDevicePointer gave for `base` on device d (0: not asked yet); filled by the caller of hold(), dies with the entry
        std::atomic<uintptr_t> device_base[kMaxDevices];
        Entry() { for (auto& d : device_base) d.store(0, std::memory_order_relaxed); }
    };

    explicit HostAdmission(const HostPinBackend& b) : be_(b) {}
    ~HostAdmission() { for (Entry* e : v_) delete e; }   // (the memory itself is the process's: nothing is unpinned at exit)
    HostAdmission(const HostAdmission&) = delete;
    HostAdmission& operator=(const HostAdmission&) = delete;

    int alloc(size_t bytes, void** out) {
        if (!out) return kInvalid;
        *out = nullptr;
        if (bytes == 0) return kInvalid;
        void* p = nullptr;
        if (int rc = be_.alloc(bytes, &p)) return rc;
        if (!insert(p, bytes, kAllocated)) { (void)be_.free_(p); return kInvalid; }
        *out = p;
        return kOk;
    }
    int free(void* p) {
        Entry* e = take(p, /*allocated=*/true);
        if (!e) return kInvalid;
        delete e;
        return be_.free_(p);
    }
    int add(void* p, size_t bytes) {
        if (!p || bytes == 0 || overlaps(p, bytes)) return kInvalid;
        int adopted = 0;
        if (int rc = be_.pin(p, bytes, &adopted)) return rc;   // (outside the lock: pinning takes its time)
        if (!insert(p, bytes, adopted ? kAdopted : kRegistered)) {   // another thread registered an overlapping range meanwhile
            if (!adopted) (void)be_.unpin(p);
            return kInvalid;
        }
        return kOk;
    }
    int remove(void* p) {
        Entry* e = take(p, /*allocated=*/false);
        if (!e) return kInvalid;
        const bool owned = e->kind == kRegistered;
        delete e;
        return owned ? be_.unpin(p) : kOk;
    }

    // The entry that wholly contains [p, p + bytes), held; nullptr: not admitted.
    Entry* hold(const void* p, size_t bytes) const {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        if (!p || bytes == 0 || a + bytes < a) return nullptr;
        std::shared_lock<std::shared_mutex> lk(mu_);
        auto it = std::upper_bound(v_.begin(), v_.end(), a, [](uintptr_t x, const Entry* e) { return x < e->base; });
        if (it == v_.begin()) return nullptr;
        Entry* e = *(it - 1);   // the last entry with base <= a
        if (a + bytes > e->end) return nullptr;
        e->uses.fetch_add(1, std::memory_order_acquire);
        return e;
    }
    static void release(Entry* e) { if (e) e->uses.fetch_sub(1, std::memory_order_release); }
    bool admitted(const void* p, size_t bytes) const {
        Entry* e = hold(p, bytes);
        release(e);
        return e != nullptr;
    }
    size_t size() const { std::shared_lock<std::shared_mutex> lk(mu_); return v_.size(); }

  private:
    std::vector<Entry*>::const_iterator first_ending_after(uintptr_t a) const {   // entries are disjoint: ends are sorted like bases
        return std::partition_point(v_.begin(), v_.end(), [a](const Entry* e) { return e->end <= a; });
    }
    bool overlaps_locked(uintptr_t a, uintptr_t b) const { auto it = first_ending_after(a); return it != v_.end() && (*it)->base < b; }
    bool overlaps(const void* p, size_t bytes) const {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        if (a + bytes < a) return true;
        std::shared_lock<std::shared_mutex> lk(mu_);
        return overlaps_locked(a, a + bytes);
    }
    bool insert(void* p, size_t bytes, Kind kind) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        if (a + bytes < a) return false;
        Entry* e = new Entry();
        e->base = a; e->end = a + bytes; e->kind = kind;
        std::unique_lock<std::shared_mutex> lk(mu_);
        if (overlaps_locked(a, a + bytes)) { lk.unlock(); delete e; return false; }
        v_.insert(first_ending_after(a), e);
        return true;
    }
    // removes the unheld entry that STARTS at p and is of the asked-for family; nullptr: none, another family, or held
    Entry* take(void* p, bool allocated) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        std::unique_lock<std::shared_mutex> lk(mu_);   // exclusive: no lookup runs, so no use count can rise
        auto it = std::lower_bound(v_.begin(), v_.end(), a, [](const Entry* e, uintptr_t x) { return e->base < x; });
        if (it == v_.end() || (*it)->base != a || ((*it)->kind == kAllocated) != allocated) return nullptr;
        if ((*it)->uses.load(std::memory_order_acquire) != 0) return nullptr;
        Entry* e = *it;
        v_.erase(it);
        return e;
    }

    HostPinBackend be_;
    mutable std::shared_mutex mu_;
    std::vector<Entry*> v_;   // sorted by base, disjoint
};

}  // namespace msorb
