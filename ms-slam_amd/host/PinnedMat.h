// Pinned, admitted host memory for the images an unchanged MS-SLAM hands to the extractor.
//
// The image that reaches ORBextractor::operator() is never the one the application decoded: System::TrackStereo makes a fresh
// cv::Mat per frame (System.cc:200-217: remap, resize or clone()), in a source file the integration leaves alone.  The one
// way to get THAT Mat into memory the library reads in place (msorb_host_alloc, include/msorb.h) is OpenCV's default allocator:
//
//     cv::Mat::setDefaultAllocator(msorb_host::PinnedMatAllocator::instance());      // first line of main()
//
// hipHostMalloc per frame costs far more than the frame, so the allocator sits on a pool: power-of-two size classes, blocks
// are reused and never freed on release, an optional byte budget trims idle blocks only.  Allocations below a threshold (64 KB:
// 3 x 3 matrices, descriptor Mats, keypoint-sized buffers) go to the standard allocator unchanged.
//
// Like every OpenCV-facing piece of this host layer the adaptor has been compiled against a stand-in only (tests/cv_stub_alloc),
// never against a real OpenCV.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <unordered_map>
#include <vector>

#ifndef MSORB_PINNED_POOL_ONLY   // (the pool alone needs neither OpenCV nor libmsorb.so: CPU tests define this and inject a backend)
#include <opencv2/opencv.hpp>

#include "msorb.h"
#endif

namespace msorb_host {

struct PinnedBackend {
    int (*alloc)(size_t bytes, void** out);   // 0 = ok (msorb_host_alloc)
    int (*free_)(void* p);                    // 0 = ok (msorb_host_free)
};

class PinnedPool {
  public:
    static constexpr int kMinShift = 12, kClasses = 36;   // 4 KB .. 2^47 bytes
    explicit PinnedPool(PinnedBackend be, size_t budget_bytes = 0) : be_(be), budget_(budget_bytes) {}
    ~PinnedPool() { trim_locked(0); }   // idle blocks go back; blocks still in use are their users'
    PinnedPool(const PinnedPool&) = delete;
    PinnedPool& operator=(const PinnedPool&) = delete;

    // A block of at least `bytes` bytes; nullptr when the backend has none.
    void* acquire(size_t bytes) {
        const int c = size_class(bytes);
        if (c < 0) return nullptr;
        std::lock_guard<std::mutex> lk(mu_);
        if (!idle_[c].empty()) {
            void* p = idle_[c].back();
            idle_[c].pop_back();
            idle_bytes_ -= class_bytes(c);
            live_.emplace(p, c);
            return p;
        }
        if (budget_ && held_bytes_ + class_bytes(c) > budget_) trim_locked(budget_ > class_bytes(c) ? budget_ - class_bytes(c) : 0);
        void* p = nullptr;
        if (be_.alloc(class_bytes(c), &p) != 0 || !p) return nullptr;
        backend_allocs_++;
        held_bytes_ += class_bytes(c);
        live_.emplace(p, c);
        return p;
    }
    // Back to the pool (not to the backend); false: not a block this pool handed out.
    bool release(void* p) {
        std::lock_guard<std::mutex> lk(mu_);
        auto it = live_.find(p);
        if (it == live_.end()) return false;
        const int c = it->second;
        live_.erase(it);
        idle_[c].push_back(p);
        idle_bytes_ += class_bytes(c);
        if (budget_ && held_bytes_ > budget_) trim_locked(budget_);
        return true;
    }
    bool owns(const void* p) const { std::lock_guard<std::mutex> lk(mu_); return live_.count(const_cast<void*>(p)) != 0; }
    void set_budget(size_t bytes) { std::lock_guard<std::mutex> lk(mu_); budget_ = bytes; if (budget_ && held_bytes_ > budget_) trim_locked(budget_); }
    size_t held_bytes() const { std::lock_guard<std::mutex> lk(mu_); return held_bytes_; }   // in use + idle
    size_t idle_bytes() const { std::lock_guard<std::mutex> lk(mu_); return idle_bytes_; }
    size_t backend_allocs() const { std::lock_guard<std::mutex> lk(mu_); return backend_allocs_; }
    static size_t class_bytes(int c) { return (size_t)1 << (kMinShift + c); }
    static int size_class(size_t bytes) {
        for (int c = 0; c < kClasses; c++)
            if (bytes <= class_bytes(c)) return c;
        return -1;
    }

  private:
    // frees idle blocks, largest class first, until no more than `target` bytes are held; blocks in use are never touched
    void trim_locked(size_t target) {
        for (int c = kClasses - 1; c >= 0 && held_bytes_ > target; c--)
            while (!idle_[c].empty() && held_bytes_ > target) {
                void* p = idle_[c].back();
                if (be_.free_(p) != 0) break;   // (the backend would not take it: it stays idle)
                idle_[c].pop_back();
                idle_bytes_ -= class_bytes(c);
                held_bytes_ -= class_bytes(c);
            }
    }
    PinnedBackend be_;
    mutable std::mutex mu_;
    std::vector<void*> idle_[kClasses];
    std::unordered_map<void*, int> live_;   // blocks in use -> size class
    size_t budget_ = 0, held_bytes_ = 0, idle_bytes_ = 0, backend_allocs_ = 0;
};

#ifndef MSORB_PINNED_POOL_ONLY
// cv::MatAllocator over a PinnedPool.  Mats of at least `threshold` bytes that OpenCV allocates itself (create, clone, remap and
// resize outputs) land in admitted pinned memory; smaller ones, Mats over user data and whatever the pool cannot serve go to the
// standard allocator unchanged (an image in pageable memory is simply staged by the library).
class PinnedMatAllocator : public cv::MatAllocator {
  public:
    static constexpr size_t kDefaultThreshold = 64 * 1024;
    // The process-wide allocator over a process-wide pool on msorb_host_alloc / msorb_host_free.  MSORB_PINNED_POOL_MB (read once)
    // sets the pool's byte budget; pool().set_budget() changes it.  Neither is ever destroyed: Mats may outlive static destructors.
    static PinnedMatAllocator* instance() {
        static PinnedMatAllocator* const a = [] {
            const char* mb = std::getenv("MSORB_PINNED_POOL_MB");
            auto* pool = new PinnedPool(PinnedBackend{msorb_host_alloc, msorb_host_free}, mb ? (size_t)std::atoll(mb) << 20 : 0);
            return new PinnedMatAllocator(pool);
        }();
        return a;
    }
    explicit PinnedMatAllocator(PinnedPool* pool, size_t threshold = kDefaultThreshold, cv::MatAllocator* std_allocator = cv::Mat::getStdAllocator())
        : pool_(pool), threshold_(threshold), std_(std_allocator) {}
    PinnedPool& pool() const { return *pool_; }
    size_t threshold() const { return threshold_; }

    cv::UMatData* allocate(int dims, const int* sizes, int type, void* data0, size_t* step, cv::AccessFlag flags,
                           cv::UMatUsageFlags usage) const override {
        size_t total = CV_ELEM_SIZE(type);
        for (int i = dims - 1; i >= 0; i--) total *= (size_t)sizes[i];
        void* p = data0 || total < threshold_ ? nullptr : pool_->acquire(total);
        if (!p) return std_->allocate(dims, sizes, type, data0, step, flags, usage);
        size_t s = CV_ELEM_SIZE(type);
        for (int i = dims - 1; i >= 0; i--) {   // dense steps, as the standard allocator sets them
            if (step) step[i] = s;
            s *= (size_t)sizes[i];
        }
        cv::UMatData* u = new cv::UMatData(this);
        u->data = u->origdata = static_cast<unsigned char*>(p);
        u->size = total;
        return u;
    }
    bool allocate(cv::UMatData* u, cv::AccessFlag, cv::UMatUsageFlags) const override { return u != nullptr; }
    void deallocate(cv::UMatData* u) const override {
        if (!u) return;
        pool_->release(u->origdata);
        delete u;
    }

  private:
    PinnedPool* pool_;
    size_t threshold_;
    cv::MatAllocator* std_;
};
#endif  // MSORB_PINNED_POOL_ONLY

}  // namespace msorb_host
