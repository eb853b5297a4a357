// TEST-ONLY host stand-in for the part of the HIP runtime that ms-slam_amd/csrc/hip_host.h calls, so that its per-thread scratch protocol
// can be compiled with g++ and checked on a machine without ROCm or a GPU.  The stub keeps a current device and tags every stream, event
// and allocation with the device that was current when it was created; destroying or freeing an object while another device is current
// (or an object the stub never made) aborts.  hip_stub::state() holds the record and the failure switches the tests set.
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidDevice = 101 };
struct ihipStream_t { int device; };
struct ihipEvent_t { int device; };
typedef ihipStream_t* hipStream_t;
typedef ihipEvent_t* hipEvent_t;
#define hipStreamNonBlocking 0x1
#define hipHostMallocDefault 0x0

namespace hip_stub {
struct Object {
    char kind;      // 's' stream, 'e' event, 'd' device block, 'h' pinned block
    int device;     // current at its creation
    size_t bytes;   // blocks only
};
struct State {
    int n_devices = 2;
    int current = 0;
    bool fail_set_device = false;   // every hipSetDevice fails (a runtime that has shut down)
    int fail_stream_on = -1;        // stream creation fails while this device is current
    int fail_malloc_on = -1;        // hipMalloc fails while this device is current
    std::map<const void*, Object> live;
    std::vector<Object> created;    // every creation, in order
    std::vector<Object> destroyed;  // every destruction / free, in order
};
inline State& state() {
    static State s;
    return s;
}
inline hipError_t make(void* p, char kind, size_t bytes) {
    const Object o{kind, state().current, bytes};
    state().live[p] = o;
    state().created.push_back(o);
    return hipSuccess;
}
inline hipError_t destroy(const void* p, char kind) {
    auto it = state().live.find(p);
    if (it == state().live.end() || it->second.kind != kind) {
        std::fprintf(stderr, "hip stub: '%c' object %p destroyed that is not live\n", kind, p);
        std::abort();
    }
    if (it->second.device != state().current) {
        std::fprintf(stderr, "hip stub: '%c' object of device %d destroyed with device %d current\n", kind, it->second.device,
                     state().current);
        std::abort();
    }
    state().destroyed.push_back(it->second);
    state().live.erase(it);
    return hipSuccess;
}
}  // namespace hip_stub

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stub failure"; }
inline hipError_t hipGetDeviceCount(int* n) {
    *n = hip_stub::state().n_devices;
    return hipSuccess;
}
inline hipError_t hipSetDevice(int d) {
    hip_stub::State& s = hip_stub::state();
    if (s.fail_set_device || d < 0 || d >= s.n_devices) return hipErrorInvalidDevice;
    s.current = d;
    return hipSuccess;
}
inline hipError_t hipStreamCreateWithFlags(hipStream_t* out, unsigned) {
    if (hip_stub::state().fail_stream_on == hip_stub::state().current) return hipErrorOutOfMemory;
    *out = new ihipStream_t{hip_stub::state().current};
    return hip_stub::make(*out, 's', 0);
}
inline hipError_t hipStreamDestroy(hipStream_t s) {
    const hipError_t e = hip_stub::destroy(s, 's');
    delete s;
    return e;
}
inline hipError_t hipEventCreate(hipEvent_t* out) {
    *out = new ihipEvent_t{hip_stub::state().current};
    return hip_stub::make(*out, 'e', 0);
}
inline hipError_t hipEventDestroy(hipEvent_t e) {
    const hipError_t r = hip_stub::destroy(e, 'e');
    delete e;
    return r;
}
inline hipError_t hipMalloc(void** p, size_t bytes) {
    if (hip_stub::state().fail_malloc_on == hip_stub::state().current) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes);
    return hip_stub::make(*p, 'd', bytes);
}
inline hipError_t hipFree(void* p) {
    const hipError_t e = hip_stub::destroy(p, 'd');
    std::free(p);
    return e;
}
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
    *p = std::malloc(bytes);
    return hip_stub::make(*p, 'h', bytes);
}
inline hipError_t hipHostFree(void* p) {
    const hipError_t e = hip_stub::destroy(p, 'h');
    std::free(p);
    return e;
}
