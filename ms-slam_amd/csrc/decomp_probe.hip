// Test hook (msorb_debug_decomp): the small dense decompositions ALONE on explicit records, built with the library's flags from
// the headers the kernels include (decomp_probe_device.h holds the record layouts).  The one-thread routines run one thread per
// record; the two cooperative null vectors run one workgroup per record, of the size and with the shared work of the kernel that
// calls them (256 lanes on a TvWork, 64 on an MlpnpWork), and every lane's result is compared, in bits, with lane 0's.
// tests/test_decomp_gpu.py compares all of it with the host program.
#include <string>

#include "hip_host.h"
#include "decomp_probe_device.h"

namespace {

using namespace msorb::decompprobe;

__global__ __launch_bounds__(256) void decomp_probe_kernel(int op, const double* __restrict__ in, int n, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double o[kDecompOut];
    record(op, in + (size_t)i * (size_t)in_width(op), o);
    for (int k = 0; k < kDecompOut; k++) out[(size_t)i * kDecompOut + k] = o[k];
}

__global__ __launch_bounds__(kDecompTvLanes) void decomp_probe_tv_kernel(int op, const double* __restrict__ in, double* __restrict__ out) {
    __shared__ msorb::TvWork work;
    __shared__ float x0[9];
    __shared__ int differ;
    const int g = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) differ = 0;
    float x[9];
    record_tv(work, tid, kDecompTvLanes, op, in + (size_t)g * (size_t)in_width(op), x);
    if (tid == 0)
        for (int k = 0; k < 9; k++) x0[k] = x[k];
    __syncthreads();
    bool same = true;
    for (int k = 0; k < 9; k++) same = same && __float_as_uint(x[k]) == __float_as_uint(x0[k]);
    if (!same) atomicAdd(&differ, 1);
    __syncthreads();
    if (tid < kDecompOut) out[(size_t)g * kDecompOut + tid] = tid < 9 ? (double)x0[tid] : tid == 9 ? (double)differ : 0.0;
}

__global__ __launch_bounds__(kDecompMlpnpLanes) void decomp_probe_mlpnp_kernel(int op, const double* __restrict__ in, double* __restrict__ out) {
    __shared__ msorb::MlpnpWork work;
    __shared__ double x0[12];
    __shared__ int differ;
    const int g = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) differ = 0;
    double x[12];
    record_mlpnp(work, tid, kDecompMlpnpLanes, op, in + (size_t)g * (size_t)in_width(op), x);
    if (tid == 0)
        for (int k = 0; k < 12; k++) x0[k] = x[k];
    __syncthreads();
    bool same = true;
    for (int k = 0; k < 12; k++) same = same && __double_as_longlong(x[k]) == __double_as_longlong(x0[k]);
    if (!same) atomicAdd(&differ, 1);
    __syncthreads();
    if (tid < kDecompOut) out[(size_t)g * kDecompOut + tid] = tid < 12 ? x0[tid] : tid == 12 ? (double)differ : 0.0;
}

int launch_decomp_probe(int op, const double* h_in, int n, double* h_out) {
    if (n > (1 << 20)) return MSORB_E_INVALID;
    if (n == 0) return MSORB_OK;
    const size_t n_in = (size_t)n * (size_t)in_width(op), n_out = (size_t)n * kDecompOut;
    double* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, (n_in + n_out) * sizeof(double));
    if (e != hipSuccess) return MSORB_E_HIP;
    e = hipMemcpy(d, h_in, n_in * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        if (cooperative(op) == 1) hipLaunchKernelGGL(decomp_probe_tv_kernel, dim3((unsigned)n), dim3(kDecompTvLanes), 0, 0, op, d, d + n_in);
        else if (cooperative(op) == 2) hipLaunchKernelGGL(decomp_probe_mlpnp_kernel, dim3((unsigned)n), dim3(kDecompMlpnpLanes), 0, 0, op, d, d + n_in);
        else hipLaunchKernelGGL(decomp_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, d, n, d + n_in);
        e = hipDeviceSynchronize();
    }
    if (e == hipSuccess) e = hipMemcpy(h_out, d + n_in, n_out * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? MSORB_OK : MSORB_E_HIP;
}

}  // namespace

extern "C" int msorb_debug_decomp(int device, int op, const double* in, int n, double* out) {
    if (n < 0 || op < 0 || op >= kDecompOps || (n > 0 && (!in || !out))) return MSORB_E_INVALID;
    HIPCHK(hipSetDevice(device));
    const int rc = launch_decomp_probe(op, in, n, out);
    if (rc == MSORB_E_HIP) msorb::set_last_error(std::string("msorb_debug_decomp: ") + hipGetErrorString(hipGetLastError()));
    return rc;
}
