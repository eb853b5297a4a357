// Test hook (msorb_debug_lie): the shared Lie-group primitives ALONE on explicit records, one thread per record, built with the
// library's flags from the headers the optimisers include (lie_probe_device.h holds the record layouts).  What the optimisers'
// kernels inline is this text; tests/test_lie_primitives_gpu.py compares it with the host program and an exact value.
#include <string>

#include "hip_host.h"
#include "lie_probe_device.h"

namespace {

using namespace msorb::lieprobe;

__global__ __launch_bounds__(256) void lie_probe_kernel(int op, const double* __restrict__ in, int n, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double o[kLieOut];
    record(op, in + (size_t)i * (size_t)(kLieIn * in_records(op)), o);
    for (int k = 0; k < kLieOut; k++) out[(size_t)i * kLieOut + k] = o[k];
}

int launch_lie_probe(int op, const double* h_in, int n, double* h_out) {
    if (n > (1 << 20)) return MSORB_E_INVALID;
    if (n == 0) return MSORB_OK;
    const size_t n_in = (size_t)n * (size_t)(kLieIn * in_records(op)), n_out = (size_t)n * kLieOut;
    double* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, (n_in + n_out) * sizeof(double));
    if (e != hipSuccess) return MSORB_E_HIP;
    e = hipMemcpy(d, h_in, n_in * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(lie_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, d, n, d + n_in);
        e = hipDeviceSynchronize();
    }
    if (e == hipSuccess) e = hipMemcpy(h_out, d + n_in, n_out * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? MSORB_OK : MSORB_E_HIP;
}

}  // namespace

extern "C" int msorb_debug_lie(int device, int op, const double* in, int n, double* out) {
    if (n < 0 || op < 0 || op >= kLieOps || (n > 0 && (!in || !out))) return MSORB_E_INVALID;
    HIPCHK(hipSetDevice(device));
    const int rc = launch_lie_probe(op, in, n, out);
    if (rc == MSORB_E_HIP) msorb::set_last_error(std::string("msorb_debug_lie: ") + hipGetErrorString(hipGetLastError()));
    return rc;
}
