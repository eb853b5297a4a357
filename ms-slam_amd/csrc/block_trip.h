// One staged block of an entry point and its trip through the calling thread's stream (hip_host.h ThreadScratch): the layout of
// the block's regions and the chain [upload | fill | launch | download | synchronise] that every BoW-node search runs.  Not part
// of the C ABI; nothing in it belongs to one entry, so other host paths can call it too.
#pragma once
#include "hip_host.h"

namespace msorb {

// The regions of one staged block, taken in order at 16-byte offsets: the inputs (uploaded in one piece) first, the outputs behind.
struct BlockLayout {
    size_t end = 0, in_bytes = 0;
    size_t take(size_t bytes) { const size_t o = end; end += up16(bytes); return o; }
    void outputs_begin() { in_bytes = end; }
};

// pinned host <-> device on a stream by the copy kernel (orb_kernels.hip; hipMemcpyAsync for unaligned pointers /
// MSORB_FRAME_COPIES=sdma): a block of 100-300 KB is across before an SDMA copy has started
hipError_t small_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s);

// One trip through scr's stream: [upload | fill_bytes set to 0xFF (-1 as int; none when 0) | launch(stream) | download |
// synchronise], the launch between scr.ev[0] and scr.ev[1] when elapsed_ms is asked for.  A HIP error is reported under `what`
// and releases scr (the stream may hold the failed work): the next call starts clean.
struct BlockTrip {
    void* d_in; const void* h_in; size_t in_bytes;
    void* d_fill; size_t fill_bytes;
    void* h_out; const void* d_out; size_t out_bytes;
};
template <class Launch>
int round_trip(ThreadScratch& scr, const char* what, const BlockTrip& t, float* elapsed_ms, Launch launch) {
    hipStream_t s = scr.s;
    hipError_t e = small_copy(t.d_in, t.h_in, t.in_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && t.fill_bytes) e = hipMemsetAsync(t.d_fill, 0xFF, t.fill_bytes, s);
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[0], s);
    if (e == hipSuccess) { launch(s); e = hipGetLastError(); }
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[1], s);
    if (e == hipSuccess) e = small_copy(t.h_out, t.d_out, t.out_bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && elapsed_ms) e = hipEventElapsedTime(elapsed_ms, scr.ev[0], scr.ev[1]);
    if (e == hipSuccess) return MSORB_OK;
    set_last_error(std::string(what) + ": " + hipGetErrorString(e));
    scr.release();
    return MSORB_E_HIP;
}

}  // namespace msorb
