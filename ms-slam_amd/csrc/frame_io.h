// Per-frame I/O of the extractor entries, as plain arithmetic (no HIP): the one block a frame's outputs travel back in, and which
// plane of the handle's pinned staging block an image of a two-image call goes through.  tests/frame_io_main.cc runs both on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/msorb.h"

namespace msorb {

// The output block of a two-image call: [kps 2*cap][desc 2*cap*32], and with the stereo fields behind them
// [u_right cap][depth cap][n_oob][n_left][n_right].  The same layout on the device and in pinned memory: one copy brings it back.
struct FrameBlock {
    size_t cap, kp_bytes, o_desc, o_ur = 0, o_dp = 0, o_oob = 0, o_cnt = 0, out_bytes;
    FrameBlock(int capacity, bool stereo) : cap((size_t)capacity), kp_bytes(cap * sizeof(msorb_keypoint)), o_desc(2 * kp_bytes), out_bytes(o_desc + 2 * cap * 32) {
        if (!stereo) return;
        o_ur = out_bytes;
        o_dp = o_ur + cap * 4;
        o_oob = o_dp + cap * 4;
        o_cnt = o_oob + 4;
        out_bytes = o_oob + 16;
    }
    size_t o_kps(int image) const { return (size_t)image * kp_bytes; }
    size_t o_descs(int image) const { return o_desc + (size_t)image * cap * 32; }
    // The tail of a call: the counts n[2] against the library's capacity (a negative count) and the caller's, then the copies out of the
    // block o in pinned memory; u_right / depth / n_oob only where the block has them.  -> nullptr, or the text of MSORB_E_CAPACITY.
    const char* copy_out(const uint8_t* o, const int n[2], int caller_capacity, msorb_keypoint* const kps[2], uint8_t* const desc[2],
                         float* u_right, float* depth, int* n_oob) const {
        if (n[0] < 0 || n[1] < 0) return "keypoint capacity exceeded";
        if (n[0] > caller_capacity || n[1] > caller_capacity) return "caller capacity too small";
        for (int i = 0; i < 2; i++) memcpy(kps[i], o + o_kps(i), (size_t)n[i] * sizeof(msorb_keypoint));
        for (int i = 0; i < 2; i++) memcpy(desc[i], o + o_descs(i), (size_t)n[i] * 32);
        if (!o_ur) return nullptr;
        memcpy(u_right, o + o_ur, (size_t)n[0] * sizeof(float));
        memcpy(depth, o + o_dp, (size_t)n[0] * sizeof(float));
        if (n_oob) memcpy(n_oob, o + o_oob, sizeof(int));
        return nullptr;
    }
};

// msorb_extract_pair: a staged image may lie in THIS handle's own staging block (msorb_stage_image stages into plane 0 of the two
// planes at `block`): the plane an un-staged image is copied into must not be one a staged image of the call still has to be
// uploaded from.  dst_plane[i]: the plane image i is staged into (or its host level 0 goes to) if it has no `staged` bit.
// -> nullptr, or why the call is refused (MSORB_E_INVALID).
inline const char* pair_staging_planes(const uint8_t* block, size_t plane, size_t pitch, const uint8_t* const src[2], const size_t stride[2],
                                       int staged, int dst_plane[2]) {
    int own_plane[2] = {-1, -1};   // plane of the block a staged image occupies (overlaps), -1: memory of another handle
    for (int i = 0; i < 2; i++) {
        if (!(staged & (1 << i))) continue;
        if (stride[i] != pitch) return "msorb_extract_pair: a staged image must have the staging pitch";
        if (src[i] + plane > block && src[i] < block + 2 * plane) {
            if (src[i] != block && src[i] != block + plane)
                return "msorb_extract_pair: a staged pointer inside this handle's staging block must be a plane msorb_stage_image returned";
            own_plane[i] = src[i] == block ? 0 : 1;
        }
    }
    for (int i = 0; i < 2; i++) dst_plane[i] = own_plane[1 - i] == i ? 1 - i : i;   // the partner's staged image sits in this image's usual plane: take the other one
    return nullptr;
}

}  // namespace msorb
