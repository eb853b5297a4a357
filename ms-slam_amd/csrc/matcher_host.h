// Internals shared by the host-side matcher sources (matcher_host.hip, track.hip): the frame handle (features + 64x48
// grid on the device) and the device rounds of the claiming window search (its replay rule: claim_replay.h).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "claim_replay.h"
#include "hip_host.h"
#include "matcher_device.h"
#include "matcher_rules.h"
#include "orb_device.h"

namespace msorb {
int extractor_last_view(msorb_extractor* h, PyramidView* pyr, LevelScale* sc, float* inv_scale, int* device,
                        hipStream_t* stream, int* n_images);
int extractor_device(const msorb_extractor* h);
int extractor_levels(const msorb_extractor* h);
bool extractor_force_peer_pyramid(const msorb_extractor* h);   // MSORB_FORCE_PEER_PYRAMID at the handle's creation (test hook)
}  // namespace msorb
struct msorb_frame_track;
namespace msorb {
void frame_track_release(msorb_frame* f);
int frame_host_grid(msorb_frame* f);
int frame_grid_max_keypoints();        // largest keypoint count the device grid takes on the current device (-1: query failed)
void frame_invalidate(msorb_frame* f);  // a failed set leaves the handle empty, never half new / half old
// sets the frame's device side (train arrays + grid) from device arrays: enqueue only, on stream s (track.hip)
// the motion-model projection that rides the frame's grid launch (track.hip frame_grid_kernel): `prepare` fills the kernel's
// LastFrameArgs (behind `args`) once the frame's fields are set, right before the launch
struct LastFrameProjector {
    int (*prepare)(void* ctx, hipStream_t s, void* args);
    void* ctx;
};
int enqueue_frame_from_device(msorb_frame* f, hipStream_t s, const msorb_keypoint* d_kps, const uint8_t* d_desc,
                              const float* d_u_right, const int* d_count, int n_fixed, int n_cap, float min_x, float max_x,
                              float min_y, float max_y, const float* scale_factors, int nlevels, const LastFrameProjector* proj = nullptr);
}  // namespace msorb

struct msorb_frame {
    int device = 0;
    hipStream_t stream = nullptr;
    int N = 0, nlevels = 0;
    float minX = 0, minY = 0, maxX = 0, maxY = 0, gridWInv = 0, gridHInv = 0;
    std::vector<msorb_keypoint> kps;
    std::vector<float> u_right, scale;
    std::vector<int> cell_begin, cell_idx;
    msorb::DevBuf<msorb::KpLite> d_kp;
    msorb::DevBuf<uint8_t> d_desc, d_occ, d_qdesc, d_stage, d_win;   // d_win: queries | descriptors | occupancy of a host-fed window search, one upload
    msorb::DevBuf<int> d_cell_begin, d_cell_idx, d_n;
    msorb::DevBuf<int> d_init_cnt, d_init_beg;   // msorb_search_for_initialization: candidate counts / list offsets / lists
    msorb::DevBuf<int2> d_init_list;
    int last_rounds = 0;                // device rounds of the last claim-replaying search (msorb_frame_search_rounds)
    long long total_rounds = 0, total_searches = 0;
    bool host_grid_valid = false;       // cell_begin / cell_idx (host) mirror the device grid
    std::mutex grid_mu;                 // the lazy fetch of that mirror (msorb_frame_features_in_area is a const query)
    msorb_frame_track* track = nullptr;  // staging of the local-points chain (track.hip)
    msorb::DevBuf<msorb::WinQuery> d_q;
    msorb::DevBuf<msorb::TopK> d_topk;
    msorb::PinBuf<uint8_t> h_in;    // queries + query descriptors + occupancy, staged
    msorb::PinBuf<msorb::TopK> h_topk;
    msorb::FrameView view() const {
        msorb::FrameView v;
        v.kp = d_kp.p; v.desc = d_desc.p; v.cell_begin = d_cell_begin.p; v.cell_idx = d_cell_idx.p;
        v.occupied = d_occ.p; v.minX = minX; v.minY = minY; v.gridWInv = gridWInv; v.gridHInv = gridHInv; v.n = N;
        for (int l = 0; l < MSORB_MAX_LEVELS; l++) v.inv_sigma2[l] = 0.0f;
        v.gate_kp = nullptr;
        return v;
    }
};


namespace msorb {

inline HostGrid host_grid(const msorb_frame* f) {   // valid after frame_host_grid(f)
    return HostGrid{f->kps.data(), f->cell_begin.data(), f->cell_idx.data(), f->minX, f->minY, f->gridWInv, f->gridHInv};
}

// Device side of one frame's claiming window search: what a round of the replay (claim_replay.h) runs.
//   q / qdesc   host queries + descriptors to upload; nullptr: f->d_q / f->d_qdesc already hold them (built on the device)
//   d_qdesc     device query descriptors when they do not live in f->d_qdesc
//   lanes       lanes per query of the window kernel (0: chosen from the mean radius of the host queries)
// A frame without keypoints has no device side: prepare and round do nothing.
struct WindowRounds {
    msorb_frame* f = nullptr;
    int M = 0, lanes = 0;
    const WinQuery* q_dev = nullptr;
    const uint8_t* d_qdesc = nullptr;
    uint8_t *occ_dev = nullptr, *h_occ = nullptr;
    size_t block_bytes = 0;   // host queries + host descriptors: queries | descriptors staged ahead of the occupancy, pending as ONE upload
                              // that the first round() issues (and zeroes this): such a search has no round 0 run by the caller

    int prepare(msorb_frame* frame, int n_queries, const WinQuery* q, const uint8_t* qdesc, const uint8_t* qdesc_dev, int n_lanes) {
        f = frame; M = n_queries; lanes = n_lanes; d_qdesc = qdesc_dev;
        if (f->N <= 0) return MSORB_OK;
        int rc;
        if ((rc = f->d_q.ensure(M)) || (!d_qdesc && (rc = f->d_qdesc.ensure((size_t)M * 32))) || (rc = f->d_topk.ensure(M)) ||
            (rc = f->d_occ.ensure(f->N)))
            return rc;
        // host queries + host descriptors (the class paths: ORBmatcher::SearchByProjection with unchanged callers): queries, descriptors
        // and the occupancy snapshot are staged side by side and go up as ONE copy into one device block (three copy launches before:
        // each costs the host ~6 us to issue and the chain ~3 us)
        const bool one_block = q && qdesc && !d_qdesc;
        if (!d_qdesc) d_qdesc = f->d_qdesc.p;
        hipStream_t s = f->stream;
        const size_t qb = q ? (size_t)M * sizeof(WinQuery) : 0, db = qdesc ? (size_t)M * 32 : 0;
        const size_t qb16 = (qb + 15) & ~(size_t)15;
        if ((rc = f->h_in.ensure(qb16 + db + (size_t)f->N + 64)) || (rc = f->h_topk.ensure(M))) return rc;
        if (one_block && (rc = f->d_win.ensure(qb16 + db + (size_t)f->N + 64))) return rc;
        q_dev = one_block ? reinterpret_cast<const WinQuery*>(f->d_win.p) : f->d_q.p;
        if (one_block) d_qdesc = f->d_win.p + qb16;
        occ_dev = one_block ? f->d_win.p + qb16 + db : f->d_occ.p;
        h_occ = f->h_in.p + qb16 + db;
        if (lanes == 0) {   // lanes per query from the mean window radius of the valid queries
            lanes = 16;
            if (q) {
                double sum = 0;
                int nv = 0;
                for (int i = 0; i < M; i++)
                    if (q[i].flags & kQValid) { sum += q[i].r; nv++; }
                if (nv) lanes = window_lanes_for((float)(sum / nv), f->gridWInv, f->gridHInv);
            }
        }
        if (q) std::memcpy(f->h_in.p, q, qb);
        if (qdesc) std::memcpy(f->h_in.p + qb16, qdesc, db);
        if (one_block) block_bytes = qb16 + db;
        else {
            if (q) HIPCHK(small_copy(f->d_q.p, f->h_in.p, qb, hipMemcpyHostToDevice, s));
            if (qdesc) HIPCHK(small_copy(f->d_qdesc.p, f->h_in.p + qb16, db, hipMemcpyHostToDevice, s));
        }
        return MSORB_OK;
    }
    // the lists of queries [from, M) against the occupancy occ, into f->h_topk (stream synchronised)
    int round(const uint8_t* occ, int from) {
        if (f->N <= 0) return MSORB_OK;
        hipStream_t s = f->stream;
        std::memcpy(h_occ, occ, f->N);  // the previous round's copy has completed (stream synchronised below)
        if (block_bytes) {
            HIPCHK(small_copy(f->d_win.p, f->h_in.p, block_bytes + (size_t)f->N, hipMemcpyHostToDevice, s));   // queries | descriptors | occupancy
            block_bytes = 0;
        } else
            HIPCHK(small_copy(occ_dev, h_occ, f->N, hipMemcpyHostToDevice, s));
        FrameView view = f->view();
        view.occupied = occ_dev;
        launch_window_topk(view, q_dev, d_qdesc, from, M, f->d_topk.p, s, 1, 0, 0, nullptr, lanes);
        HIPCHK(small_copy(f->h_topk.p + from, f->d_topk.p + from, (size_t)(M - from) * sizeof(TopK), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return MSORB_OK;
    }
    ClaimSide side(const WinQuery* q, const uint8_t* flags, uint8_t* occ) const {
        ClaimSide S;
        S.kps = f->kps.data(); S.N = f->N; S.q = q; S.flags = flags; S.topk = f->h_topk.p; S.occ = occ;
        return S;
    }
    void account(int rounds) const { f->last_rounds = rounds; f->total_rounds += rounds; f->total_searches++; }   // msorb_frame_search_rounds
};

// One-camera claiming window search: replay_claims (claim_replay.h) over the device rounds of frame f.
//   flags       kQValid / kQSkipOccupied per query; nullptr: taken from q
//   ready       round 0 has been run by the caller: f->d_occ holds `occ`, f->h_topk[0, M) the lists (stream synchronised)
// q / qdesc / d_qdesc / lanes as WindowRounds takes them, accept as replay_claims takes it.
template <typename Accept>
int run_window_search(msorb_frame* f, int M, const WinQuery* q, const uint8_t* flags, const uint8_t* qdesc,
                      std::vector<uint8_t>& occ, int need, Accept accept, bool ready = false, int* rounds_out = nullptr,
                      const uint8_t* d_qdesc = nullptr, int lanes = 0) {
    if (rounds_out) *rounds_out = 0;
    if (M <= 0 || f->N <= 0) return MSORB_OK;   // no queries / no train keypoints (also a handle whose set failed): no match
    if (!flags && !q) return MSORB_E_INVALID;
    if (ready && q && qdesc && !d_qdesc) {   // a round 0 of the caller's cannot have read queries that are still to go up
        set_last_error("run_window_search: ready with host queries and host descriptors");
        return MSORB_E_INVALID;
    }
    WindowRounds dev;
    if (const int rc = dev.prepare(f, M, q, qdesc, d_qdesc, lanes)) return rc;
    ClaimSide S = dev.side(q, flags, occ.data());
    const int rounds = replay_claims(S, M, need, ready, [&](int from) { return dev.round(occ.data(), from); }, accept);
    if (rounds < 0) return rounds;
    if (rounds_out) *rounds_out = rounds;
    dev.account(rounds);
    return MSORB_OK;
}

}  // namespace msorb
