// msorb_ldlt_solve: the blocked L D L^T of ldlt_blocked.h on host arrays (upload, solve, read-back), so that the solver can be
// tested alone; msorb_ldlt_block_sizes tells the tests where its paths change.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/msorb.h"
#include "hip_host.h"
#include "ldlt_blocked.h"

using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::up16;
namespace ldlt = msorb::ldlt;

extern "C" int msorb_ldlt_block_sizes(int* panel, int* tile) {
    if (!panel || !tile) return MSORB_E_ARG;
    *panel = ldlt::kNB;
    *tile = ldlt::kTile;
    return MSORB_OK;
}

extern "C" int msorb_ldlt_solve(int device, int n, const double* S, const double* b, double* x, int* ok, float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (n < 1 || !S || !b || !x || !ok) return MSORB_E_ARG;
    if (int rc = msorb::require_device(device)) return rc;
    const size_t nn = (size_t)n * n * 8, nv = (size_t)n * 8;
    const size_t o_S = 0, o_b = up16(nn), o_x = o_b + up16(nv), o_ws = o_x + up16(nv);
    const size_t o_ok = o_ws + up16(ldlt::workspace_doubles(n) * 8), dev_bytes = o_ok + 16;
    static thread_local ThreadScratch scr(true, 2);
    if (int rc = scr.acquire(device, dev_bytes, up16(nv) + 16)) return rc;   // pinned: x and the flag; S and b go up from the caller's pages
    uint8_t *const d = scr.d.p, *const h = scr.h.p;
    hipStream_t s = scr.s;
    ldlt::Work W{};
    W.n = n;
    W.S = reinterpret_cast<double*>(d + o_S);
    W.b = reinterpret_cast<const double*>(d + o_b);
    W.x = reinterpret_cast<double*>(d + o_x);
    ldlt::carve_workspace(W, reinterpret_cast<double*>(d + o_ws));
    W.ok = reinterpret_cast<int*>(d + o_ok);
    hipError_t err = hipSuccess;
    auto fail = [&](const char* what) {
        set_last_error(std::string("ldlt_solve: ") + what + ": " + hipGetErrorString(err));
        scr.release();
        return MSORB_E_HIP;
    };
#define LDLT_TRY(expr) do { err = (expr); if (err != hipSuccess) return fail(#expr); } while (0)
    LDLT_TRY(hipMemcpyAsync(d + o_S, S, nn, hipMemcpyHostToDevice, s));
    LDLT_TRY(hipMemcpyAsync(d + o_b, b, nv, hipMemcpyHostToDevice, s));
    LDLT_TRY(hipEventRecord(scr.ev[0], s));
    LDLT_TRY(ldlt::launch(W, s));
    LDLT_TRY(hipEventRecord(scr.ev[1], s));
    LDLT_TRY(hipMemcpyAsync(h, d + o_x, nv, hipMemcpyDeviceToHost, s));
    LDLT_TRY(hipMemcpyAsync(h + up16(nv), d + o_ok, 4, hipMemcpyDeviceToHost, s));
    LDLT_TRY(hipStreamSynchronize(s));
    if (elapsed_ms) LDLT_TRY(hipEventElapsedTime(elapsed_ms, scr.ev[0], scr.ev[1]));
#undef LDLT_TRY
    int flag;
    std::memcpy(&flag, h + up16(nv), 4);
    *ok = flag != 0;
    if (*ok) std::memcpy(x, h, nv);   // a failed pivot: the device's x was never written, the caller's stays as it is
    return MSORB_OK;
}
