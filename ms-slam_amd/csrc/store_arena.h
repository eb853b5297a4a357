// What the device-resident stores (the KeyFrame store of bow_match.hip, the BoW database of kf_database.hip) share: the offsets
// of their arenas and the grow-and-carry-over of a device array.  Not part of the C ABI.
#ifndef MSORB_STORE_ARENA_H
#define MSORB_STORE_ARENA_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <iterator>
#include <map>

namespace msorb {

// Offsets inside one of a store's arenas (feature rows; FeatureVector entries; BowVector entries): first fit over the free ranges,
// neighbours merged on release, the arena's end pulled back when its last range is released.  A KeyFrame that is removed (culled,
// compacted by map sparsification, evicted) gives its rows back — a sequence inserts and culls KeyFrames for as long as it runs
// (tests/soak_main.cc: 268 MB after 100 000 frames when removed rows stayed allocated).
struct RangeAlloc {
    size_t end = 0;                    // first offset past the highest range in use
    std::map<size_t, size_t> free_;    // offset -> length, disjoint, non-adjacent, all below `end`
    size_t take(size_t n) {
        if (n == 0) return 0;
        for (auto it = free_.begin(); it != free_.end(); ++it)
            if (it->second >= n) {
                const size_t off = it->first, rest = it->second - n;
                free_.erase(it);
                if (rest) free_[off + n] = rest;
                return off;
            }
        const size_t off = end;
        end += n;
        return off;
    }
    void give(size_t off, size_t n) {
        if (n == 0) return;
        auto nx = free_.lower_bound(off);
        if (nx != free_.begin()) {
            auto pv = std::prev(nx);
            if (pv->first + pv->second == off) { off = pv->first; n += pv->second; free_.erase(pv); }
        }
        if (nx != free_.end() && off + n == nx->first) { n += nx->second; free_.erase(nx); }
        if (off + n == end) end = off;
        else free_[off] = n;
    }
    size_t free_total() const { size_t t = 0; for (auto& e : free_) t += e.second; return t; }
};

// p[cap * unit] -> at least p[need * unit], the first `used * unit` elements carried over (the device is current)
template <class T>
hipError_t grow(T*& p, size_t used, size_t& cap, size_t need, size_t unit) {
    if (need <= cap) return hipSuccess;
    const size_t ncap = std::max(need, cap * 2 + 4096);
    T* q = nullptr;
    hipError_t e = hipMalloc((void**)&q, ncap * unit * sizeof(T));
    if (e != hipSuccess) return e;
    if (p && used) e = hipMemcpy(q, p, used * unit * sizeof(T), hipMemcpyDeviceToDevice);
    if (p) (void)hipFree(p);
    p = q;
    cap = ncap;
    return e;
}

}  // namespace msorb
#endif
