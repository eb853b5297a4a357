// Host-side helpers of the entry points (no kernels): the HIP error macro, the device check, grow-only device / pinned buffers and
// the per-calling-thread scratch of the entries that run once per frame or per call.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/msorb.h"

namespace msorb {
void set_last_error(const std::string& s);
}

#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            msorb::set_last_error(std::string(#expr) + ": " + hipGetErrorString(_e));          \
            return MSORB_E_HIP;                                                                \
        }                                                                                      \
    } while (0)

namespace msorb {

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// A device ordinal the runtime does not have is an error (libmsorb has no CPU fallback).  The device is not made current here.
inline int require_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        set_last_error("no usable HIP device (libmsorb has no CPU fallback)");
        return MSORB_E_NO_DEVICE;
    }
    return MSORB_OK;
}

// Grow-only buffers: ensure() keeps the block while it is large enough and otherwise replaces it (the contents are not kept).
// + 16 bytes: small_copy moves whole 16-byte units.  No destructor: the owner releases them with their device current.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    int ensure(size_t count) {
        if (count <= n) return MSORB_OK;
        release();
        HIPCHK(hipMalloc((void**)&p, count * sizeof(T) + 16));
        n = count;
        return MSORB_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};
// pinned host staging: hipMemcpyAsync from / to pageable memory makes the driver stage and synchronise per call
template <typename T>
struct PinBuf {
    T* p = nullptr;
    size_t n = 0;
    int ensure(size_t count) {
        if (count <= n) return MSORB_OK;
        release();
        HIPCHK(hipHostMalloc((void**)&p, count * sizeof(T) + 16, hipHostMallocDefault));
        n = count;
        return MSORB_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
};

// Scratch of one calling thread (a `static thread_local` of an entry point), bound to one device at a time: a stream if asked for,
// n_events events, one grow-only device block and one grow-only pinned block (1.5x headroom), which the caller carves at 16-byte
// offsets.  acquire(dev, ...) returns with dev current.  A device other than the last call's releases the old state with the old
// device current and creates everything anew on dev; `device` records dev only once all of it exists, and any failure releases what
// was made, so the next call starts clean.
struct ThreadScratch {
    const bool with_stream;
    const int n_events;
    int device = -1;
    hipStream_t s = nullptr;
    hipEvent_t ev[4] = {};   // n_events <= 4
    DevBuf<uint8_t> d;
    PinBuf<uint8_t> h;

    ThreadScratch(bool stream, int events) : with_stream(stream), n_events(events) {}
    ~ThreadScratch() { release(); }
    ThreadScratch(const ThreadScratch&) = delete;
    ThreadScratch& operator=(const ThreadScratch&) = delete;

    int acquire(int dev, size_t dev_bytes, size_t pin_bytes) {
        if (dev != device) release();
        HIPCHK(hipSetDevice(dev));
        const int rc = create_and_grow(dev_bytes, pin_bytes);
        if (rc != MSORB_OK) {
            drop(true);   // (dev is current)
            return rc;
        }
        device = dev;
        return MSORB_OK;
    }
    // frees everything with its device current; when that device cannot be made current (a runtime that has shut down, at thread
    // exit) nothing is freed
    void release() { drop(device >= 0 && hipSetDevice(device) == hipSuccess); }

  private:
    int create_and_grow(size_t dev_bytes, size_t pin_bytes) {
        if (device < 0) {
            if (with_stream) HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
            for (int i = 0; i < n_events; i++) HIPCHK(hipEventCreate(&ev[i]));
        }
        int rc;
        if (dev_bytes > d.n && (rc = d.ensure(dev_bytes + dev_bytes / 2))) return rc;
        if (pin_bytes > h.n && (rc = h.ensure(pin_bytes + pin_bytes / 2))) return rc;
        return MSORB_OK;
    }
    void drop(bool free) {
        if (free) {
            d.release();
            h.release();
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
            if (s) (void)hipStreamDestroy(s);
        }
        d = {};
        h = {};
        for (hipEvent_t& e : ev) e = nullptr;
        s = nullptr;
        device = -1;
    }
};

}  // namespace msorb
