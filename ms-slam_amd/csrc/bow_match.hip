// ORBmatcher::SearchByBoW (src/ORBmatcher.cc:223-421 pinhole branch, :872-1016, :1018-1166) for a batch of
// (KeyFrame, Frame) / (KeyFrame, KeyFrame) pairs.
//
// The reference merge-walks the two DBoW2::FeatureVectors (:239-243, :385-392); for every node both have, each
// query of the node (in list order) scans the node's trains that are still unclaimed (:274-275, :937), keeps
// best / second best with strict '<' (:283-292) and, when accepted (:332-336), claims its best train.  A feature
// sits in exactly one node of its vector, so claims never cross nodes: the nodes are independent problems and the
// order dependence lives inside one node only.  Here: one wavefront per (pair, common node); the node's trains are
// spread over the lanes (position p = chunk*64 + lane, chunk 0's descriptors stay in registers), the node's queries
// are visited in list order, each one a wave-wide masked top-2 (key = dist<<20 | position, so the minimum is the
// first strict minimum of the reference's scan), the claim is one bit in LDS.  The rotation histogram and
// ComputeThreeMaxima (:340-353, :396-418) run on the host for the per-call entries (bow_pairs.h), on the device for resident KeyFrames.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/msorb.h"
#include "block_trip.h"
#include "bow_pairs.h"
#include "hip_host.h"
#include "matcher_device.h"
#include "matcher_rules.h"
#include "new_points_device.h"
#include "store_arena.h"

using msorb::set_last_error;
using msorb::kHistoLength;
using msorb::ThreadScratch;
using msorb::BlockLayout;
using msorb::BlockTrip;
using msorb::round_trip;
using msorb::FeatVec;
using msorb::check_feature_vector;

namespace {

struct BowItem {  // one (pair, common node)
    int base1, base2;  // first row of the pair's set 1 / set 2 in the descriptor (and static per-feature) arrays
    int b1, n1l;       // the node's query list inside feat1
    int b2, n2l;       // the node's train list inside feat2
    int pair;
    int m1, m2;        // first entry of the pair's set 1 / set 2 in the PER-CALL arrays (visit / availability flags, match12):
                       // equal to base1 / base2 when everything is staged per call, different when the descriptors live in a
                       // resident KeyFrame store
};

__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

constexpr int kNoKey = 0x7fffffff;

__global__ __launch_bounds__(64) void bow_match_kernel(const BowItem* __restrict__ items, const uint4* __restrict__ desc1,
                                                       const uint4* __restrict__ desc2, const uint8_t* __restrict__ valid1,
                                                       const uint8_t* __restrict__ avail2, const int* __restrict__ feat1,
                                                       const int* __restrict__ feat2, int th_low, int flags,
                                                       float nnratio, int* __restrict__ match12, int* __restrict__ best1 = nullptr) {
    // flags: bit 0 = inclusive (best <= th_low, :332; else best < th_low, :959), bit 1 = no ratio test (the right-camera arm of
    // SearchByBoW(pKF, F) on a two-camera frame, :357-359: `|| true`).  best1 (optional): per query feature the distance of its best
    // unclaimed train at the time it is processed — before the threshold and the ratio test — or 256.
    const int inclusive = flags & 1;
    const bool no_ratio = (flags & 2) != 0;
    extern __shared__ unsigned free_bits[];  // bit p: train at list position p is unclaimed
    const BowItem it = items[blockIdx.x];
    const int lane = threadIdx.x;
    const int chunks = (it.n2l + 63) >> 6;
    for (int w = lane; w < chunks * 2; w += 64) free_bits[w] = 0;
    __syncthreads();
    uint4 t0 = make_uint4(0, 0, 0, 0), t1 = t0;
    for (int c = 0; c < chunks; c++) {
        const int p = c * 64 + lane;
        bool fr = false;
        if (p < it.n2l) {
            const int f2 = feat2[it.b2 + p], idx2 = it.base2 + f2;
            fr = avail2[it.m2 + f2] != 0;
            if (c == 0) { t0 = desc2[(size_t)idx2 * 2]; t1 = desc2[(size_t)idx2 * 2 + 1]; }
        }
        const unsigned long long m = __ballot(fr);
        if (lane == 0) { free_bits[2 * c] = (unsigned)m; free_bits[2 * c + 1] = (unsigned)(m >> 32); }
    }
    __syncthreads();
    for (int k1 = 0; k1 < it.n1l; k1++) {
        const int f1 = feat1[it.b1 + k1], idx1 = it.base1 + f1;
        if (!valid1[it.m1 + f1]) continue;  // wave uniform
        const uint4 q0 = desc1[(size_t)idx1 * 2], q1 = desc1[(size_t)idx1 * 2 + 1];
        int key = kNoKey, second = 256;
        for (int c = 0; c < chunks; c++) {
            const int p = c * 64 + lane;
            if (p < it.n2l && ((free_bits[p >> 5] >> (p & 31)) & 1u)) {
                int dist;
                if (c == 0) dist = hamming256(q0, q1, t0, t1);
                else {
                    const int idx2 = it.base2 + feat2[it.b2 + p];
                    dist = hamming256(q0, q1, desc2[(size_t)idx2 * 2], desc2[(size_t)idx2 * 2 + 1]);
                }
                if (dist < 256) {  // bestDist1 starts at 256 with a strict '<' (:265-267, :283)
                    const int kk = (dist << 20) | p;
                    if (kk < key) { second = min(second, key >> 20); key = kk; }
                    else second = min(second, dist);
                }
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int ok = __shfl_xor(key, off), os = __shfl_xor(second, off);
            second = min(min(second, os), max(key, ok) >> 20);
            key = min(key, ok);
        }
        second = min(second, 256);
        const int best = key >> 20;
        if (best1 && lane == 0) best1[it.m1 + f1] = key != kNoKey ? best : 256;
        const bool pass = key != kNoKey && (inclusive ? best <= th_low : best < th_low) &&
                          (no_ratio || (float)best < nnratio * (float)second);  // :332-336, :959-961
        if (pass) {
            const int p = key & 0xFFFFF;
            if (lane == 0) {
                match12[it.m1 + f1] = feat2[it.b2 + p];
                free_bits[p >> 5] &= ~(1u << (p & 31));
            }
            __syncthreads();
        }
    }
}

struct TriConst {  // per pair
    float F[9];
    float ep[2];
};

// SearchForTriangulation's node problem (:1230-1358): best-only, bestDist starts at TH_LOW and a candidate replaces
// the best when dist <= bestDist (:1277) — the LAST minimum of the scan — provided it passes the epipole-distance
// gate (:1283-1291, mono-mono only) and Pinhole::epipolarConstrain (Pinhole.cpp:107-131).  The gates do not depend on
// the running best, so the winner is the minimum of key = dist<<20 | (0xFFFFF - position) over the gated candidates.
__global__ __launch_bounds__(64) void triangulation_match_kernel(
    const BowItem* __restrict__ items, const TriConst* __restrict__ consts, const uint4* __restrict__ desc1,
    const uint4* __restrict__ desc2, const uint8_t* __restrict__ flags1, const uint8_t* __restrict__ flags2,
    const float2* __restrict__ xy1, const float4* __restrict__ tr2, const int* __restrict__ feat1,
    const int* __restrict__ feat2, int coarse, int* __restrict__ match12) {
    extern __shared__ unsigned free_bits[];
    const BowItem it = items[blockIdx.x];
    const TriConst K = consts[it.pair];
    const int lane = threadIdx.x;
    const int chunks = (it.n2l + 63) >> 6;
    for (int w = lane; w < chunks * 2; w += 64) free_bits[w] = 0;
    __syncthreads();
    uint4 t0 = make_uint4(0, 0, 0, 0), t1 = t0;
    float4 r0 = make_float4(0, 0, 0, 0);
    bool s0 = false;
    for (int c = 0; c < chunks; c++) {
        const int p = c * 64 + lane;
        bool fr = false;
        if (p < it.n2l) {
            const int f2 = feat2[it.b2 + p], idx2 = it.base2 + f2;
            const uint8_t fl = flags2[it.m2 + f2];
            fr = (fl & 1) != 0;
            if (c == 0) { t0 = desc2[(size_t)idx2 * 2]; t1 = desc2[(size_t)idx2 * 2 + 1]; r0 = tr2[idx2]; s0 = (fl & 2) != 0; }
        }
        const unsigned long long m = __ballot(fr);
        if (lane == 0) { free_bits[2 * c] = (unsigned)m; free_bits[2 * c + 1] = (unsigned)(m >> 32); }
    }
    __syncthreads();
    for (int k1 = 0; k1 < it.n1l; k1++) {
        const int f1 = feat1[it.b1 + k1], idx1 = it.base1 + f1;
        const uint8_t fl1 = flags1[it.m1 + f1];
        if (!(fl1 & 1)) continue;  // wave uniform
        const bool stereo1 = (fl1 & 2) != 0;
        const uint4 q0 = desc1[(size_t)idx1 * 2], q1 = desc1[(size_t)idx1 * 2 + 1];
        const float2 P1 = xy1[idx1];
        // l = x1' F12 (Pinhole.cpp:114-117)
        const float a = __fadd_rn(__fmaf_rn(P1.x, K.F[0], __fmul_rn(P1.y, K.F[3])), K.F[6]);
        const float b = __fadd_rn(__fmaf_rn(P1.x, K.F[1], __fmul_rn(P1.y, K.F[4])), K.F[7]);
        const float cc = __fadd_rn(__fmaf_rn(P1.x, K.F[2], __fmul_rn(P1.y, K.F[5])), K.F[8]);
        const float den = __fmaf_rn(a, a, __fmul_rn(b, b));
        int key = kNoKey;
        for (int c = 0; c < chunks; c++) {
            const int p = c * 64 + lane;
            if (p < it.n2l && ((free_bits[p >> 5] >> (p & 31)) & 1u)) {
                int dist;
                float4 r;
                bool stereo2;
                if (c == 0) { dist = hamming256(q0, q1, t0, t1); r = r0; stereo2 = s0; }
                else {
                    const int f2 = feat2[it.b2 + p], idx2 = it.base2 + f2;
                    dist = hamming256(q0, q1, desc2[(size_t)idx2 * 2], desc2[(size_t)idx2 * 2 + 1]);
                    r = tr2[idx2];
                    stereo2 = (flags2[it.m2 + f2] & 2) != 0;
                }
                bool ok = dist <= msorb::kThLow;  // :1277
                if (ok && !stereo1 && !stereo2) {  // :1283-1291
                    const float ex = __fsub_rn(K.ep[0], r.x), ey = __fsub_rn(K.ep[1], r.y);
                    if (__fmaf_rn(ex, ex, __fmul_rn(ey, ey)) < r.z) ok = false;
                }
                if (ok && !coarse) {  // Pinhole.cpp:119-130
                    const float num = __fadd_rn(__fmaf_rn(a, r.x, __fmul_rn(b, r.y)), cc);
                    if (den == 0.0f) ok = false;
                    else {
                        const float dsqr = __fdiv_rn(__fmul_rn(num, num), den);
                        ok = (double)dsqr < 3.84 * (double)r.w;
                    }
                }
                if (ok) key = min(key, (dist << 20) | (0xFFFFF - p));
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) key = min(key, __shfl_xor(key, off));
        if (key != kNoKey) {
            const int p = 0xFFFFF - (key & 0xFFFFF);
            if (lane == 0) {
                match12[it.m1 + f1] = feat2[it.b2 + p];
                free_bits[p >> 5] &= ~(1u << (p & 31));
            }
            __syncthreads();
        }
    }
}

// Every (query, train) of a node with distance <= th_low among the visited queries / eligible trains, in the reference's scan order
// (queries in list order, trains in list order): the candidates of a search whose accept test lives with the CALLER
// (msorb_search_for_triangulation_cb: GeometricCamera::epipolarConstrain of a camera model this library does not hold).
// FILL = false counts per item, FILL = true writes (query, train, dist, train position) at list + begin[item].
template <bool FILL>
__global__ __launch_bounds__(64) void node_candidates_kernel(const BowItem* __restrict__ items, const uint4* __restrict__ desc1,
                                                             const uint4* __restrict__ desc2, const uint8_t* __restrict__ valid1,
                                                             const uint8_t* __restrict__ avail2, const int* __restrict__ feat1,
                                                             const int* __restrict__ feat2, int th_low, int* __restrict__ count,
                                                             const int* __restrict__ begin, int4* __restrict__ list) {
    const BowItem it = items[blockIdx.x];
    const int lane = threadIdx.x;
    const int chunks = (it.n2l + 63) >> 6;
    int total = 0;
    int4* out = FILL ? list + begin[blockIdx.x] : nullptr;
    for (int k1 = 0; k1 < it.n1l; k1++) {
        const int f1 = feat1[it.b1 + k1];
        if (!valid1[it.m1 + f1]) continue;  // wave uniform
        const int idx1 = it.base1 + f1;
        const uint4 q0 = desc1[(size_t)idx1 * 2], q1 = desc1[(size_t)idx1 * 2 + 1];
        for (int c = 0; c < chunks; c++) {
            const int p = c * 64 + lane;
            bool ok = false;
            int f2 = 0, dist = 0;
            if (p < it.n2l) {
                f2 = feat2[it.b2 + p];
                if (avail2[it.m2 + f2]) {
                    const int idx2 = it.base2 + f2;
                    dist = hamming256(q0, q1, desc2[(size_t)idx2 * 2], desc2[(size_t)idx2 * 2 + 1]);
                    ok = dist <= th_low;
                }
            }
            const unsigned long long m = __ballot(ok);
            if (FILL && ok) out[total + __popcll(m & ((1ull << lane) - 1))] = make_int4(f1, f2, dist, p);
            total += __popcll(m);
        }
    }
    if (!FILL && lane == 0) count[blockIdx.x] = total;
}

// The rotation-consistency filter of a pair on the device (resident-KeyFrame entries): histogram of round((angle1 - angle2) / 12
// degrees) over the pair's raw matches, ComputeThreeMaxima (ORBmatcher.cc:2277-2318) on the 30 counts, matches outside the
// three fullest bins withdrawn (:396-418, :1360-1381), match21 and the count written.  The survivors do not depend on the
// order the reference visits the matches in — only the counts enter — so no replay on the host is needed (the host loop
// over 2000 features costs 24 us per pair: seven times the device part of a 32-pair batch).  One workgroup per pair.
struct PairPost {
    int m1, n1, m2, n2;   // the pair's slices of the per-call match12 / match21 arrays
    int a1, a2;           // first entry of the pair's set 1 / set 2 in angle1 / angle2
};
__global__ __launch_bounds__(256) void pair_histogram_kernel(const PairPost* __restrict__ posts, const float* __restrict__ angle1,
                                                            const float* __restrict__ angle2, int check_orientation,
                                                            int* __restrict__ match12, int* __restrict__ match21,
                                                            int* __restrict__ nmatches) {
    __shared__ int hist[kHistoLength];
    __shared__ int ind[3];
    __shared__ int total;
    const PairPost P = posts[blockIdx.x];
    const int t = threadIdx.x;
    if (t < kHistoLength) hist[t] = 0;
    if (t == 0) total = 0;
    __syncthreads();
    auto bin_of = [&](int i, int idx2) {
        float rot = __fsub_rn(angle1[P.a1 + i], angle2[P.a2 + idx2]);
        if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
        int bin = (int)roundf(__fmul_rn(rot, 1.0f / kHistoLength));
        if (bin == kHistoLength) bin = 0;
        return (bin >= 0 && bin < kHistoLength) ? bin : -1;   // NaN / out-of-range angle: the reference asserts
    };
    if (check_orientation) {
        for (int i = t; i < P.n1; i += 256) {
            const int idx2 = match12[P.m1 + i];
            if (idx2 < 0) continue;
            const int b = bin_of(i, idx2);
            if (b >= 0) atomicAdd(&hist[b], 1);
        }
        __syncthreads();
        if (t == 0) {
            int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
            for (int i = 0; i < kHistoLength; i++) {
                const int s = hist[i];
                if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
                else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
                else if (s > max3) { max3 = s; i3 = i; }
            }
            if (max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
            else if (max3 < 0.1f * (float)max1) { i3 = -1; }
            ind[0] = i1; ind[1] = i2; ind[2] = i3;
        }
        __syncthreads();
    }
    int kept = 0;
    for (int i = t; i < P.n1; i += 256) {
        const int idx2 = match12[P.m1 + i];
        if (idx2 < 0) continue;
        bool keep = true;
        if (check_orientation) {
            const int b = bin_of(i, idx2);
            keep = b >= 0 && (b == ind[0] || b == ind[1] || b == ind[2]);
        }
        if (!keep) { match12[P.m1 + i] = -1; continue; }
        kept++;
        if (match21 && idx2 < P.n2) match21[P.m2 + idx2] = i;
    }
    atomicAdd(&total, kept);
    __syncthreads();
    if (t == 0) nmatches[blockIdx.x] = total;
}

// ------------------------------------------------------------------------------------------------------------------
// Host side.  Every entry goes through the same four stages: validate its pairs, walk their FeatureVectors into
// (pair, common node) items (NodeWork), lay out and stage one pinned block (BlockLayout), run it through the stream
// (round_trip).  What is plain C++ about two FeatureVectors and a match list is in bow_pairs.h.
// ------------------------------------------------------------------------------------------------------------------

// A set of a pair has its FeatureVector lists either in a device array that holds the whole vector (a resident KeyFrame, the
// frame block of a call: feat = where the vector's feat[0] sits in that array) or among the lists this call stages, the common
// nodes' lists one behind the other (kStaged).
constexpr int kStaged = INT32_MIN;

struct NodeWork {   // the items of one call
    std::vector<BowItem> items;
    std::vector<std::pair<const int*, const int*>> lists;   // per item: its staged query / train list on the host
    size_t totf1 = 0, totf2 = 0;                            // staged list entries
    int max_chunks = 1;

    // appends the items of pair pi (BowItem: base1 / base2, m1 / m2); false: a train list too long for the kernels
    bool add(const FeatVec& a, const FeatVec& b, int pi, int base1, int base2, int m1, int m2, int feat1 = kStaged, int feat2 = kStaged) {
        return msorb::for_each_common_node(a, b, max_chunks, [&](int r1, int r2, int l1, int l2) {
            const int b1 = feat1 == kStaged ? (int)totf1 : feat1 + a.begin[r1], b2 = feat2 == kStaged ? (int)totf2 : feat2 + b.begin[r2];
            items.push_back(BowItem{base1, base2, b1, l1, b2, l2, pi, m1, m2});
            lists.push_back({feat1 == kStaged ? a.feat + a.begin[r1] : nullptr, feat2 == kStaged ? b.feat + b.begin[r2] : nullptr});
            if (feat1 == kStaged) totf1 += (size_t)l1;
            if (feat2 == kStaged) totf2 += (size_t)l2;
        });
    }
    size_t item_bytes() const { return items.size() * sizeof(BowItem); }
    void stage(void* h_items, int* f1, int* f2) const {
        std::memcpy(h_items, items.data(), item_bytes());
        for (size_t i = 0; i < items.size(); i++) {
            if (lists[i].first) std::memcpy(f1 + items[i].b1, lists[i].first, (size_t)items[i].n1l * 4);
            if (lists[i].second) std::memcpy(f2 + items[i].b2, lists[i].second, (size_t)items[i].n2l * 4);
        }
    }
    dim3 grid() const { return dim3((unsigned)items.size()); }
    size_t lds() const { return (size_t)max_chunks * 8; }   // one bit per train of the longest list
};

template <class P> FeatVec fv1_of(const P& p) { return FeatVec{p.fv1_nodes, p.fv1_node, p.fv1_begin, p.fv1_feat}; }
template <class P> FeatVec fv2_of(const P& p) { return FeatVec{p.fv2_nodes, p.fv2_node, p.fv2_begin, p.fv2_feat}; }

bool check_bow_pair(const msorb_bow_pair& P, int check_orientation, bool need_match12, std::vector<uint8_t>& seen) {
    return P.n1 >= 0 && P.n2 >= 0 && (P.match12 || !need_match12 || P.n1 == 0) && (P.n1 == 0 || (P.desc1 && P.valid1)) &&
           (P.n2 == 0 || P.desc2) && (!check_orientation || ((P.n1 == 0 || P.angle1) && (P.n2 == 0 || P.angle2))) &&
           check_feature_vector(P.n1, fv1_of(P), seen) && check_feature_vector(P.n2, fv2_of(P), seen);
}

void stage_flags(uint8_t* dst, const uint8_t* flags, size_t n) {   // nullptr: every feature
    if (flags) std::memcpy(dst, flags, n);
    else std::memset(dst, 1, n);
}
void stage_const(TriConst& c, const float* F12, const float* ep) {
    std::memcpy(c.F, F12, sizeof(c.F));
    c.ep[0] = ep[0];
    c.ep[1] = ep[1];
}

// The inputs of the per-call SearchByBoW forms (msorb_search_by_bow, msorb_search_for_triangulation_cb): validation, walk, and the
// regions [desc1 | desc2 | feat1 | feat2 | items | valid1 | avail2] of the block.
struct BowCall {
    NodeWork w;
    size_t tot1 = 0, tot2 = 0;
    size_t o_d1, o_d2, o_f1, o_f2, o_it, o_v1, o_a2;
    BlockLayout L;

    // validates and walks the pairs (-1 or the first bad pair), sets every match12 / match21 to -1
    int walk(msorb_bow_pair* pairs, int n_pairs, int check_orientation) {
        std::vector<uint8_t> seen;
        for (int pi = 0; pi < n_pairs; pi++) {
            msorb_bow_pair& P = pairs[pi];
            P.nmatches = 0;
            if (!check_bow_pair(P, check_orientation, true, seen) ||
                !w.add(fv1_of(P), fv2_of(P), pi, (int)tot1, (int)tot2, (int)tot1, (int)tot2)) return pi;
            tot1 += (size_t)P.n1;
            tot2 += (size_t)P.n2;
        }
        for (int pi = 0; pi < n_pairs; pi++) {
            std::fill_n(pairs[pi].match12, pairs[pi].n1, -1);
            if (pairs[pi].match21) std::fill_n(pairs[pi].match21, pairs[pi].n2, -1);
        }
        return -1;
    }
    void plan() {
        o_d1 = L.take(tot1 * 32); o_d2 = L.take(tot2 * 32); o_f1 = L.take(w.totf1 * 4); o_f2 = L.take(w.totf2 * 4);
        o_it = L.take(w.item_bytes()); o_v1 = L.take(tot1); o_a2 = L.take(tot2);
        L.outputs_begin();
    }
    void stage(uint8_t* h, const msorb_bow_pair* pairs, int n_pairs) const {
        size_t r1 = 0, r2 = 0;
        for (int pi = 0; pi < n_pairs; pi++) {
            const msorb_bow_pair& P = pairs[pi];
            if (P.n1) { std::memcpy(h + o_d1 + r1 * 32, P.desc1, (size_t)P.n1 * 32); std::memcpy(h + o_v1 + r1, P.valid1, (size_t)P.n1); }
            if (P.n2) { std::memcpy(h + o_d2 + r2 * 32, P.desc2, (size_t)P.n2 * 32); stage_flags(h + o_a2 + r2, P.avail2, (size_t)P.n2); }
            r1 += (size_t)P.n1;
            r2 += (size_t)P.n2;
        }
        w.stage(h + o_it, (int*)(h + o_f1), (int*)(h + o_f2));
    }
};

// The raw matches of a call are read feature by feature: out of the pinned block first (one streaming copy) — scattered 4-byte
// reads of pinned host memory cost ~10 ns each, 0.8 ms for a 32-pair batch.
const int* out_of_pinned(const void* pinned, size_t n) {
    static thread_local std::vector<int> m_local;
    m_local.resize(n);
    std::memcpy(m_local.data(), pinned, n * 4);
    return m_local.data();
}

// a pair's raw matches (the kernel's; -1 where no feature was matched or visited) through the rotation filter into match12 / match21;
// angles(i1, i2, a1, a2) = the angles of the two keypoints
template <class Angles>
int finish_pair(int n1, const int* raw, int check_orientation, int* match12, int* match21, Angles angles) {
    if (n1) std::memcpy(match12, raw, (size_t)n1 * 4);
    const int nm = msorb::rotation_filter(n1, check_orientation, match12, [&](int i) { return raw[i] >= 0 ? i : -1; },
                                          [&](int i, float& a1, float& a2) { angles(i, raw[i], a1, a2); });
    if (match21)
        for (int i = 0; i < n1; i++)
            if (match12[i] >= 0) match21[match12[i]] = i;
    return nm;
}
// (a per-call SearchByBoW pair keeps its angles in two arrays)
int finish_bow_pair(msorb_bow_pair& P, const int* raw, int check_orientation) {
    return finish_pair(P.n1, raw, check_orientation, P.match12, P.match21,
                       [&](int i1, int i2, float& a1, float& a2) { a1 = P.angle1[i1]; a2 = P.angle2[i2]; });
}

void launch_bow(hipStream_t s, const NodeWork& w, const uint8_t* d_items, const uint4* desc1, const uint4* desc2, const uint8_t* valid1,
                const uint8_t* avail2, const int* feat1, const int* feat2, int th_low, int flags, float nnratio, uint8_t* match12,
                uint8_t* best1 = nullptr) {
    hipLaunchKernelGGL(bow_match_kernel, w.grid(), dim3(64), w.lds(), s, (const BowItem*)d_items, desc1, desc2, valid1, avail2, feat1,
                       feat2, th_low, flags, nnratio, (int*)match12, (int*)best1);
}

// msorb_search_by_bow's body.  flags: bit 0 inclusive, bit 1 no ratio test; best1 (optional): per pair the kernel's best1 output.
int search_by_bow_impl(int device, msorb_bow_pair* pairs, int n_pairs, int th_low, int flags, float nnratio, int check_orientation,
                       float* elapsed_ms, std::vector<std::vector<int>>* best1) {
    if (best1) { best1->assign(n_pairs, {}); for (int pi = 0; pi < n_pairs; pi++) (*best1)[pi].assign(std::max(pairs[pi].n1, 0), 256); }
    if (elapsed_ms) *elapsed_ms = 0;
    if (n_pairs < 0 || (n_pairs > 0 && !pairs)) return MSORB_E_INVALID;
    if (n_pairs == 0) return MSORB_OK;
    BowCall c;
    const int bad = c.walk(pairs, n_pairs, check_orientation);
    if (bad >= 0) {
        set_last_error("search_by_bow: pair " + std::to_string(bad) +
                       ": bad sizes / null arrays / feature vector not ascending, out of range or with a repeated feature");
        return MSORB_E_INVALID;
    }
    if (c.w.items.empty()) return MSORB_OK;
    const size_t tot1 = c.tot1;
    if (tot1 > (size_t)INT32_MAX / 2 || c.tot2 > (size_t)INT32_MAX / 2) return MSORB_E_INVALID;
    if (int rc = msorb::require_device(device)) return rc;
    c.plan();   // [match12 | best1] out
    const size_t o_m = c.L.take(tot1 * 4), o_b = best1 ? c.L.take(tot1 * 4) : c.L.end;
    static thread_local ThreadScratch scr(true, 2);
    if (int rc = scr.acquire(device, c.L.end, c.L.end)) return rc;
    uint8_t *h = scr.h.p, *d = scr.d.p;
    c.stage(h, pairs, n_pairs);
    const BlockTrip trip{d, h, c.L.in_bytes, d + o_m, tot1 * 4, h + o_m, d + o_m, (best1 ? o_b - o_m : 0) + tot1 * 4};
    if (int rc = round_trip(scr, "search_by_bow", trip, elapsed_ms, [&](hipStream_t s) {
            launch_bow(s, c.w, d + c.o_it, (const uint4*)(d + c.o_d1), (const uint4*)(d + c.o_d2), d + c.o_v1, d + c.o_a2,
                       (const int*)(d + c.o_f1), (const int*)(d + c.o_f2), th_low, flags, nnratio, d + o_m, best1 ? d + o_b : nullptr);
        })) return rc;
    if (best1)   // written for the visited features only (the valid ones of the common nodes): the others keep 256
        for (size_t k = 0; k < c.w.items.size(); k++) {
            const BowItem& it = c.w.items[k];
            for (int q = 0; q < it.n1l; q++) {
                const int i1 = c.w.lists[k].first[q];
                if (pairs[it.pair].valid1[i1]) (*best1)[it.pair][i1] = ((const int*)(h + o_b))[it.m1 + i1];
            }
        }
    const int* raw = out_of_pinned(h + o_m, tot1);
    for (int pi = 0; pi < n_pairs; pi++) {
        pairs[pi].nmatches = finish_bow_pair(pairs[pi], raw, check_orientation);
        raw += pairs[pi].n1;
    }
    return MSORB_OK;
}

}  // namespace

extern "C" int msorb_search_by_bow(int device, msorb_bow_pair* pairs, int n_pairs, int th_low, int inclusive, float nnratio,
                                   int check_orientation, float* elapsed_ms) {
    return search_by_bow_impl(device, pairs, n_pairs, th_low, inclusive ? 1 : 0, nnratio, check_orientation, elapsed_ms, nullptr);
}

// ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) on a two-camera frame (F.Nleft != -1), ORBmatcher.cc:223-421 with the arms of
// :276-309 and :357-382: inside a BoW node every KeyFrame feature keeps a best / second over the frame's LEFT features and a best
// over its RIGHT features (rows >= n_left), both among the features no earlier KeyFrame feature has claimed.  The left match is
// taken as on a one-camera frame (<= TH_LOW, ratio test); the right match — only looked at when the LEFT best distance was <= TH_LOW,
// whatever the ratio test said (:330 encloses :357) — is taken at <= TH_LOW without a ratio test (`|| true`).  Left and right claims
// touch disjoint features, so the two arms are two runs of the node kernel: the left one also reports every KeyFrame feature's
// left best distance, which gates the right one.  Both feed ONE rotation histogram (:338-353, :361-378, :396-418).
//   pair: as msorb_search_by_bow (set 1 = the KeyFrame, set 2 = the frame's n2 = N features, left camera first; avail2 unused);
//   match21[n2]: the KeyFrame feature matched to frame feature j (vpMapPointMatches[j] = its map point), -1 none.
extern "C" int msorb_search_by_bow_rig(int device, msorb_bow_pair* pair, int n_left, int th_low, float nnratio, int check_orientation) {
    if (!pair || n_left < 0 || n_left > pair->n2 || !pair->match21) return MSORB_E_INVALID;
    msorb_bow_pair& P = *pair;
    P.nmatches = 0;
    std::vector<uint8_t> seen;
    if (!check_bow_pair(P, check_orientation, false, seen)) {
        set_last_error("search_by_bow_rig: bad sizes / null arrays / feature vector not ascending, out of range or with a repeated feature");
        return MSORB_E_INVALID;
    }
    const msorb::CameraSplit cam = msorb::split_by_camera(fv2_of(P), n_left);
    std::vector<int> m12L(std::max(P.n1, 1), -1), m12R(std::max(P.n1, 1), -1);
    auto arm = [&](const FeatVec& fv2, const uint8_t* valid1, int* match12) {
        msorb_bow_pair A = P;
        A.valid1 = valid1; A.avail2 = nullptr; A.match12 = match12; A.match21 = nullptr;
        A.fv2_nodes = fv2.nodes; A.fv2_node = fv2.node; A.fv2_begin = fv2.begin; A.fv2_feat = fv2.feat;
        return A;
    };
    msorb_bow_pair A = arm(cam.left.view(), P.valid1, m12L.data());
    std::vector<std::vector<int>> best1;
    int rc = search_by_bow_impl(device, &A, 1, th_low, 1, nnratio, 0, nullptr, &best1);
    if (rc) return rc;
    std::vector<uint8_t> validR(std::max(P.n1, 1), 0);
    for (int i = 0; i < P.n1; i++) validR[i] = P.valid1[i] && best1[0][i] <= th_low;                // :330
    msorb_bow_pair B = arm(cam.right.view(), validR.data(), m12R.data());
    rc = search_by_bow_impl(device, &B, 1, th_low, 1 | 2, nnratio, 0, nullptr, nullptr);
    if (rc) return rc;
    // two entries per KeyFrame feature, its left match and its right match, into the one histogram
    auto partner = [&](int k) { return (k & 1 ? m12R : m12L)[k >> 1]; };
    std::fill_n(P.match21, P.n2, -1);
    for (int k = 0; k < 2 * P.n1; k++)
        if (partner(k) >= 0) P.match21[partner(k)] = k >> 1;
    P.nmatches = msorb::rotation_filter(2 * P.n1, check_orientation, P.match21, partner,
                                        [&](int k, float& a1, float& a2) { a1 = P.angle1[k >> 1]; a2 = P.angle2[partner(k)]; });
    if (P.match12) {   // the left partner of every KeyFrame feature (the right one is in match21 only)
        std::fill_n(P.match12, P.n1, -1);
        for (int f2 = 0; f2 < n_left; f2++) if (P.match21[f2] >= 0) P.match12[P.match21[f2]] = f2;
    }
    return MSORB_OK;
}

// ORBmatcher::SearchForTriangulation (:1168-1402) with the geometric test of :1332 left to the caller — the form the two-camera arms
// (:1294-1330: one of four relative poses and two camera models per candidate, KannalaBrandt8::epipolarConstrain) need, and any
// camera model this library does not restate.  The device lists, per common node, every (query, train) within th_low among the
// visited / eligible features (node_candidates_kernel: count, then fill); msorb::pick_candidates replays the reference's scan over
// them.  accept() is a pure predicate of the two features (the reference's is: a const camera, two keypoints, a relative pose), so
// asking it for fewer or other candidates than the reference's running-minimum scan reaches changes nothing.
extern "C" int msorb_search_for_triangulation_cb(int device, msorb_bow_pair* pair, int th_low, int check_orientation, msorb_pair_accept accept,
                                                 void* ctx) {
    if (!pair || !accept || th_low < 0) return MSORB_E_INVALID;
    msorb_bow_pair& P = *pair;
    BowCall c;
    if (c.walk(pair, 1, check_orientation) >= 0) {
        set_last_error("search_for_triangulation_cb: bad sizes / null arrays / feature vector not ascending, out of range or with a repeated feature");
        return MSORB_E_INVALID;
    }
    const size_t n_items = c.w.items.size();
    if (n_items == 0) return MSORB_OK;
    if (int rc = msorb::require_device(device)) return rc;
    c.plan();   // [count] out, [begin] in for the second trip; the lists in their own block
    const size_t o_cnt = c.L.take(n_items * 4), o_beg = c.L.take(n_items * 4);
    static thread_local ThreadScratch scr(true, 2), lists(true, 2);
    if (int rc = scr.acquire(device, c.L.end, c.L.end)) return rc;
    uint8_t *h = scr.h.p, *d = scr.d.p;
    c.stage(h, pair, 1);
    auto launch = [&](auto kernel, hipStream_t s) {
        hipLaunchKernelGGL(kernel, c.w.grid(), dim3(64), 0, s, (const BowItem*)(d + c.o_it), (const uint4*)(d + c.o_d1),
                           (const uint4*)(d + c.o_d2), (const uint8_t*)(d + c.o_v1), (const uint8_t*)(d + c.o_a2), (const int*)(d + c.o_f1),
                           (const int*)(d + c.o_f2), th_low, (int*)(d + o_cnt), (const int*)(d + o_beg), (int4*)lists.d.p);
    };
    const BlockTrip count{d, h, c.L.in_bytes, nullptr, 0, h + o_cnt, d + o_cnt, n_items * 4};
    if (int rc = round_trip(scr, "search_for_triangulation_cb", count, nullptr, [&](hipStream_t s) { launch(node_candidates_kernel<false>, s); }))
        return rc;
    const int* cnt = (const int*)(h + o_cnt);
    int* beg = (int*)(h + o_beg);
    size_t n_cand = 0;
    for (size_t i = 0; i < n_items; i++) { beg[i] = (int)n_cand; n_cand += (size_t)cnt[i]; }
    std::vector<int> raw((size_t)P.n1, -1);
    if (n_cand > 0) {
        if (n_cand > (size_t)INT32_MAX / 16) { set_last_error("search_for_triangulation_cb: too many candidates"); return MSORB_E_CAPACITY; }
        if (int rc = lists.acquire(device, n_cand * sizeof(int4), n_cand * sizeof(int4))) return rc;
        const BlockTrip fill{d + o_beg, beg, n_items * 4, nullptr, 0, lists.h.p, lists.d.p, n_cand * sizeof(int4)};
        if (int rc = round_trip(scr, "search_for_triangulation_cb", fill, nullptr, [&](hipStream_t s) { launch(node_candidates_kernel<true>, s); }))
            return rc;
        static_assert(sizeof(msorb::NodeCand) == sizeof(int4), "node_candidates_kernel writes int4");
        std::vector<msorb::NodeCand> all((const msorb::NodeCand*)lists.h.p, (const msorb::NodeCand*)lists.h.p + n_cand);   // (out of the pinned block: read repeatedly)
        std::vector<uint8_t> matched2((size_t)P.n2, 0);
        msorb::pick_candidates(all.data(), n_cand, matched2.data(), raw.data(), [&](int i1, int i2) { return accept(ctx, i1, i2) != 0; });
    }
    P.nmatches = finish_bow_pair(P, raw.data(), check_orientation);
    return MSORB_OK;
}

namespace {
void launch_triangulation(hipStream_t s, const NodeWork& w, const uint8_t* d_items, const uint8_t* d_consts, const uint4* desc1,
                          const uint4* desc2, const uint8_t* flags1, const uint8_t* flags2, const float2* xy1, const float4* tr2,
                          const int* feat1, const int* feat2, int coarse, uint8_t* match12) {
    hipLaunchKernelGGL(triangulation_match_kernel, w.grid(), dim3(64), w.lds(), s, (const BowItem*)d_items, (const TriConst*)d_consts,
                       desc1, desc2, flags1, flags2, xy1, tr2, feat1, feat2, coarse, (int*)match12);
}
}  // namespace

extern "C" int msorb_search_for_triangulation(int device, msorb_triangulation_pair* pairs, int n_pairs, int coarse,
                                              int check_orientation, float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (n_pairs < 0 || (n_pairs > 0 && !pairs)) return MSORB_E_INVALID;
    if (n_pairs == 0) return MSORB_OK;
    NodeWork w;
    std::vector<uint8_t> seen;
    size_t tot1 = 0, tot2 = 0;
    for (int pi = 0; pi < n_pairs; pi++) {
        msorb_triangulation_pair& P = pairs[pi];
        P.nmatches = 0;
        bool ok = P.n1 >= 0 && P.n2 >= 0 && (P.n1 == 0 || (P.match12 && P.desc1 && P.valid1 && P.stereo1 && P.kp1)) &&
                  (P.n2 == 0 || (P.desc2 && P.avail2 && P.stereo2 && P.kp2 && P.scale_factors2 && P.level_sigma2_2 &&
                                 P.n_levels2 > 0));
        for (int j = 0; ok && j < P.n2; j++) ok = P.kp2[j].octave >= 0 && P.kp2[j].octave < P.n_levels2;
        if (!ok || !check_feature_vector(P.n1, fv1_of(P), seen) || !check_feature_vector(P.n2, fv2_of(P), seen) ||
            !w.add(fv1_of(P), fv2_of(P), pi, (int)tot1, (int)tot2, (int)tot1, (int)tot2)) {
            set_last_error("search_for_triangulation: pair " + std::to_string(pi) +
                           ": bad sizes / null arrays / octave out of range / feature vector not ascending, out of range or "
                           "with a repeated feature");
            return MSORB_E_INVALID;
        }
        tot1 += (size_t)P.n1;
        tot2 += (size_t)P.n2;
    }
    for (int pi = 0; pi < n_pairs; pi++) std::fill_n(pairs[pi].match12, pairs[pi].n1, -1);
    if (w.items.empty()) return MSORB_OK;
    if (tot1 > (size_t)INT32_MAX / 2 || tot2 > (size_t)INT32_MAX / 2) return MSORB_E_INVALID;
    if (int rc = msorb::require_device(device)) return rc;
    // [desc1 | desc2 | tr2 (x, y, 100*scale, sigma2) | xy1 | feat1 | feat2 | items | consts | flags1 | flags2] in, [match12] out
    BlockLayout L;
    const size_t o_d1 = L.take(tot1 * 32), o_d2 = L.take(tot2 * 32), o_t2 = L.take(tot2 * 16), o_x1 = L.take(tot1 * 8),
                 o_f1 = L.take(w.totf1 * 4), o_f2 = L.take(w.totf2 * 4), o_it = L.take(w.item_bytes()),
                 o_c = L.take((size_t)n_pairs * sizeof(TriConst)), o_v1 = L.take(tot1), o_a2 = L.take(tot2);
    L.outputs_begin();
    const size_t o_m = L.take(tot1 * 4);
    static thread_local ThreadScratch scr(true, 2);
    if (int rc = scr.acquire(device, L.end, L.end)) return rc;
    uint8_t *h = scr.h.p, *d = scr.d.p;
    size_t r1 = 0, r2 = 0;
    for (int pi = 0; pi < n_pairs; pi++) {
        const msorb_triangulation_pair& P = pairs[pi];
        if (P.n1) std::memcpy(h + o_d1 + r1 * 32, P.desc1, (size_t)P.n1 * 32);
        if (P.n2) std::memcpy(h + o_d2 + r2 * 32, P.desc2, (size_t)P.n2 * 32);
        msorb::pack_triangulation_side(P.n1, P.kp1, nullptr, nullptr, P.valid1, P.stereo1, (float*)(h + o_x1) + 2 * r1, nullptr, h + o_v1 + r1);
        msorb::pack_triangulation_side(P.n2, P.kp2, P.scale_factors2, P.level_sigma2_2, P.avail2, P.stereo2, nullptr,
                                       (float*)(h + o_t2) + 4 * r2, h + o_a2 + r2);
        stage_const(((TriConst*)(h + o_c))[pi], P.F12, P.ep);
        r1 += (size_t)P.n1;
        r2 += (size_t)P.n2;
    }
    w.stage(h + o_it, (int*)(h + o_f1), (int*)(h + o_f2));
    const BlockTrip trip{d, h, L.in_bytes, d + o_m, tot1 * 4, h + o_m, d + o_m, tot1 * 4};
    if (int rc = round_trip(scr, "search_for_triangulation", trip, elapsed_ms, [&](hipStream_t s) {
            launch_triangulation(s, w, d + o_it, d + o_c, (const uint4*)(d + o_d1), (const uint4*)(d + o_d2), d + o_v1, d + o_a2,
                                 (const float2*)(d + o_x1), (const float4*)(d + o_t2), (const int*)(d + o_f1), (const int*)(d + o_f2),
                                 coarse, d + o_m);
        })) return rc;
    const int* raw = out_of_pinned(h + o_m, tot1);
    for (int pi = 0; pi < n_pairs; pi++) {
        msorb_triangulation_pair& P = pairs[pi];
        P.nmatches = finish_pair(P.n1, raw, check_orientation, P.match12, nullptr,
                                 [&](int i1, int i2, float& a1, float& a2) { a1 = P.kp1[i1].angle; a2 = P.kp2[i2].angle; });
        raw += P.n1;
    }
    return MSORB_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Resident KeyFrames (DESIGN.md "what comes next" of round 1: the per-call entries above spend their time staging the
// same KeyFrames again and again — 30-40 us of kernel inside ~1 ms of copies).  A KeyFrame is matched against many
// others over its life (LocalMapping::CreateNewMapPoints against 10-20 neighbours per new KeyFrame, relocalisation and
// loop candidates against the current frame), while its descriptors, keypoints and FeatureVector are fixed once
// KeyFrame::ComputeBoW has run (until map sparsification compacts it: remove + add).  The store keeps them on the
// device; a search then uploads only the visit / availability flags (1 B per feature), the (pair, common node) work
// items and, for the KeyFrame-vs-Frame form, the frame; it downloads match12.
// ------------------------------------------------------------------------------------------------------------------
using msorb::RangeAlloc;   // (store_arena.h: first fit over the free ranges of an arena)

struct msorb_kf_store {
    int device = 0;
    mutable std::shared_mutex mu;  // searches hold it shared (the buffers must not move under a running kernel), add / remove exclusive
    struct Entry {
        bool alive = false;
        int row0 = 0, n = 0, feat0 = 0, nfeat = 0;
        std::vector<int> node, begin;   // FeatureVector: node ids ascending, list r = feat[begin[r] .. begin[r+1]) (offsets relative to feat0)
        std::vector<int> feat;          // host copy of the lists
        std::vector<float> angle;
        std::vector<uint8_t> octave;    // per keypoint (msorb_create_new_map_points_kf: rides in the per-call flag byte)
        std::vector<float> scale;       // mvScaleFactors
        FeatVec fv() const { return FeatVec{(int)node.size(), node.data(), begin.data(), feat.data()}; }
    };
    std::vector<Entry> kf;
    std::vector<int> dead_ids;   // indices of `kf` whose KeyFrame was removed: handed out again by the next add
    int n_alive = 0;
    RangeAlloc rows_a, feats_a;  // which rows / FeatureVector entries of the device arrays are in use
    size_t rows_cap = 0, feats_cap = 0;
    uint4* d_desc = nullptr;    // 2 per row
    float2* d_xy = nullptr;     // keypoint position (SearchForTriangulation, set 1)
    float4* d_tr = nullptr;     // x, y, 100 * scale[octave], sigma2[octave] (SearchForTriangulation, set 2)
    float* d_angle = nullptr;   // keypoint angles (rotation histogram)
    int* d_feat = nullptr;
    const Entry* alive(int id) const { return id >= 0 && id < (int)kf.size() && kf[id].alive ? &kf[id] : nullptr; }
};

using msorb::grow;

extern "C" int msorb_kf_store_create(int device, msorb_kf_store** out) {
    if (!out) return MSORB_E_INVALID;
    *out = nullptr;
    if (int rc = msorb::require_device(device)) return rc;
    msorb_kf_store* s = new msorb_kf_store();
    s->device = device;
    *out = s;
    return MSORB_OK;
}

extern "C" void msorb_kf_store_destroy(msorb_kf_store* s) {
    if (!s) return;
    if (hipSetDevice(s->device) == hipSuccess) {
        if (s->d_desc) (void)hipFree(s->d_desc);
        if (s->d_xy) (void)hipFree(s->d_xy);
        if (s->d_tr) (void)hipFree(s->d_tr);
        if (s->d_feat) (void)hipFree(s->d_feat);
        if (s->d_angle) (void)hipFree(s->d_angle);
    }
    delete s;
}

extern "C" int msorb_kf_store_count(const msorb_kf_store* s) {
    if (!s) return MSORB_E_INVALID;
    std::shared_lock<std::shared_mutex> lk(s->mu);
    return s->n_alive;
}

extern "C" int msorb_kf_store_add(msorb_kf_store* s, int n, const msorb_keypoint* kps, const uint8_t* desc, int fv_nodes,
                                  const int* fv_node, const int* fv_begin, const int* fv_feat, const float* scale_factors,
                                  const float* level_sigma2, int n_levels, int* kf_id) {
    if (!s || !kf_id || n < 0 || (n > 0 && (!kps || !desc)) || !scale_factors || !level_sigma2 || n_levels < 1) return MSORB_E_INVALID;
    *kf_id = -1;
    FeatVec fv{fv_nodes, fv_node, fv_begin, fv_feat};
    std::vector<uint8_t> seen;
    if (!check_feature_vector(n, fv, seen)) { set_last_error("kf_store_add: feature vector not ascending, out of range or with a repeated feature"); return MSORB_E_INVALID; }
    for (int i = 0; i < n; i++)
        if (kps[i].octave < 0 || kps[i].octave >= n_levels) { set_last_error("kf_store_add: keypoint octave out of range"); return MSORB_E_INVALID; }
    const int f_lo = fv_nodes ? fv_begin[0] : 0, f_hi = fv_nodes ? fv_begin[fv_nodes] : 0, nf = f_hi - f_lo;
    std::vector<float> xy((size_t)2 * n), tr((size_t)4 * n), ang(n);
    msorb::pack_triangulation_side(n, kps, scale_factors, level_sigma2, nullptr, nullptr, xy.data(), tr.data(), nullptr);
    for (int i = 0; i < n; i++) ang[i] = kps[i].angle;
    std::unique_lock<std::shared_mutex> lk(s->mu);
    if (hipSetDevice(s->device) != hipSuccess) return MSORB_E_HIP;
    hipError_t e = hipSuccess;
    // rows / FeatureVector entries: a free range of an earlier KeyFrame first, the end of the arena otherwise
    const size_t used_rows = s->rows_a.end, used_feats = s->feats_a.end;   // what a reallocation has to carry over
    const size_t row0 = s->rows_a.take((size_t)n), feat0 = s->feats_a.take((size_t)nf);
    size_t cap2 = s->rows_cap, cap3 = s->rows_cap, cap1 = s->rows_cap, cap4 = s->rows_cap;
    e = grow(s->d_desc, used_rows, cap1, s->rows_a.end, 2);
    if (e == hipSuccess) e = grow(s->d_xy, used_rows, cap2, s->rows_a.end, 1);
    if (e == hipSuccess) e = grow(s->d_tr, used_rows, cap3, s->rows_a.end, 1);
    if (e == hipSuccess) e = grow(s->d_angle, used_rows, cap4, s->rows_a.end, 1);
    if (e == hipSuccess) s->rows_cap = std::min(std::min(cap1, cap4), std::min(cap2, cap3));
    if (e == hipSuccess) e = grow(s->d_feat, used_feats, s->feats_cap, s->feats_a.end, 1);
    if (e == hipSuccess && n) e = hipMemcpy(s->d_desc + 2 * row0, desc, (size_t)n * 32, hipMemcpyHostToDevice);
    if (e == hipSuccess && n) e = hipMemcpy(s->d_xy + row0, xy.data(), (size_t)n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && n) e = hipMemcpy(s->d_tr + row0, tr.data(), (size_t)n * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess && nf) e = hipMemcpy(s->d_feat + feat0, fv_feat + f_lo, (size_t)nf * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && n) e = hipMemcpy(s->d_angle + row0, ang.data(), (size_t)n * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        s->rows_a.give(row0, (size_t)n); s->feats_a.give(feat0, (size_t)nf);
        set_last_error(std::string("kf_store_add: ") + hipGetErrorString(e));
        return MSORB_E_HIP;
    }
    msorb_kf_store::Entry E;
    E.alive = true; E.row0 = (int)row0; E.n = n; E.feat0 = (int)feat0; E.nfeat = nf;
    E.node.assign(fv_node, fv_node + fv_nodes);
    E.begin.resize(fv_nodes + 1);
    for (int r = 0; r <= fv_nodes; r++) E.begin[r] = (fv_nodes ? fv_begin[r] : 0) - f_lo;
    E.feat.assign(fv_feat + f_lo, fv_feat + f_hi);
    E.angle = std::move(ang);
    E.octave.resize(n);
    for (int i = 0; i < n; i++) E.octave[i] = (uint8_t)std::min(kps[i].octave, 255);
    E.scale.assign(scale_factors, scale_factors + n_levels);
    s->n_alive++;
    if (!s->dead_ids.empty()) {   // ids of removed KeyFrames come back: the table does not grow with the length of the sequence
        *kf_id = s->dead_ids.back();
        s->dead_ids.pop_back();
        s->kf[*kf_id] = std::move(E);
    } else {
        s->kf.push_back(std::move(E));
        *kf_id = (int)s->kf.size() - 1;
    }
    return MSORB_OK;
}

extern "C" int msorb_kf_store_remove(msorb_kf_store* s, int kf_id) {
    if (!s) return MSORB_E_INVALID;
    std::unique_lock<std::shared_mutex> lk(s->mu);
    if (kf_id < 0 || kf_id >= (int)s->kf.size() || !s->kf[kf_id].alive) { set_last_error("kf_store_remove: unknown KeyFrame id"); return MSORB_E_INVALID; }
    msorb_kf_store::Entry& E = s->kf[kf_id];
    E.alive = false;
    s->rows_a.give((size_t)E.row0, (size_t)E.n);       // the rows and the id are free for the next add (no kernel is running: the lock is exclusive)
    s->feats_a.give((size_t)E.feat0, (size_t)E.nfeat);
    E.n = 0; E.nfeat = 0;
    std::vector<int>().swap(E.node); E.begin.assign(1, 0); std::vector<float>().swap(E.angle); std::vector<int>().swap(E.feat);
    std::vector<uint8_t>().swap(E.octave); std::vector<float>().swap(E.scale);
    s->dead_ids.push_back(kf_id);
    s->n_alive--;
    return MSORB_OK;
}

// Rows of the device arrays in use / reserved (rows of 64 + 8 + 16 + 4 bytes): a store's footprint for long-run checks.
extern "C" int msorb_kf_store_rows(const msorb_kf_store* s, size_t* rows_in_use, size_t* rows_reserved) {
    if (!s || !rows_in_use || !rows_reserved) return MSORB_E_INVALID;
    std::shared_lock<std::shared_mutex> lk(s->mu);
    *rows_in_use = s->rows_a.end - s->rows_a.free_total();
    *rows_reserved = s->rows_cap;
    return MSORB_OK;
}

namespace {
// One pair of a resident search.  Set 1 is KeyFrame A; set 2 KeyFrame B, or the call's frame (B == nullptr: n2 features staged at
// row 0 of the frame block).  m1 / m2: the pair's first entry in the per-call arrays [flags1 of pair 0 | pair 1 | ...] and
// [flags2 ...], [match12 ...] and [match21 ...].
struct KfPair {
    const msorb_kf_store::Entry *A, *B;
    int n2, m1, m2;
    int *match12, *match21, *nmatches;
    int row2() const { return B ? B->row0 : 0; }
};

struct KfCall {   // the pairs of one resident search and their items
    std::vector<KfPair> pairs;
    NodeWork w;
    size_t tot1 = 0, tot2 = 0;

    // fv2 / feat2: the FeatureVector of set 2 and where its feat[0] sits in the device array the kernel reads its lists from
    bool add(const KfPair& p, const FeatVec& fv2, int feat2) {
        pairs.push_back(p);
        KfPair& P = pairs.back();
        P.m1 = (int)tot1; P.m2 = (int)tot2;
        tot1 += (size_t)P.A->n;
        tot2 += (size_t)P.n2;
        return w.add(P.A->fv(), fv2, (int)pairs.size() - 1, P.A->row0, P.row2(), P.m1, P.m2, P.A->feat0, feat2);
    }
    bool add(const KfPair& p) { return add(p, p.B->fv(), p.B->feat0); }
    void unmatched() const {   // no common node anywhere: nothing is launched, every feature stays unmatched
        for (const KfPair& P : pairs) {
            std::fill_n(P.match12, P.A->n, -1);
            if (P.match21) std::fill_n(P.match21, P.n2, -1);
        }
    }
    void stage_posts(void* h_posts) const {
        PairPost* posts = (PairPost*)h_posts;
        for (const KfPair& P : pairs) *posts++ = PairPost{P.m1, P.A->n, P.m2, P.n2, P.A->row0, P.row2()};
    }
    void launch_histogram(hipStream_t s, const uint8_t* d_posts, const float* angle1, const float* angle2, int check_orientation,
                          uint8_t* match12, uint8_t* match21, uint8_t* nmatches) const {
        hipLaunchKernelGGL(pair_histogram_kernel, dim3((unsigned)pairs.size()), dim3(256), 0, s, (const PairPost*)d_posts, angle1, angle2,
                           check_orientation, (int*)match12, (int*)match21, (int*)nmatches);
    }
    void deliver(const uint8_t* h_m12, const uint8_t* h_m21, const uint8_t* h_nm) const {
        for (size_t pi = 0; pi < pairs.size(); pi++) {
            const KfPair& P = pairs[pi];
            if (P.A->n) std::memcpy(P.match12, h_m12 + (size_t)P.m1 * 4, (size_t)P.A->n * 4);
            if (h_m21 && P.match21 && P.n2) std::memcpy(P.match21, h_m21 + (size_t)P.m2 * 4, (size_t)P.n2 * 4);
            *P.nmatches = ((const int*)h_nm)[pi];
        }
    }
};
}  // namespace

extern "C" int msorb_search_by_bow_kf(msorb_kf_store* st, msorb_bow_kf_pair* pairs, int n_pairs, const msorb_bow_frame* frame,
                                      int th_low, int inclusive, float nnratio, int check_orientation, float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (!st || n_pairs < 0 || (n_pairs > 0 && !pairs)) return MSORB_E_INVALID;
    if (n_pairs == 0) return MSORB_OK;
    std::shared_lock<std::shared_mutex> lk(st->mu);
    std::vector<uint8_t> seen;
    FeatVec ff{0, nullptr, nullptr, nullptr};
    if (frame) {
        ff = FeatVec{frame->fv_nodes, frame->fv_node, frame->fv_begin, frame->fv_feat};
        if (frame->n < 0 || (frame->n > 0 && !frame->desc) || (check_orientation && frame->n > 0 && !frame->angle) ||
            !check_feature_vector(frame->n, ff, seen)) {
            set_last_error("search_by_bow_kf: bad frame arrays");
            return MSORB_E_INVALID;
        }
    }
    // the frame's lists are staged from its first list entry on, its descriptors at row 0 of the frame block
    const int fr_feat_lo = ff.nodes ? ff.begin[0] : 0;
    const size_t fr_rows = frame ? (size_t)frame->n : 0, fr_feats = ff.nodes ? (size_t)(ff.begin[ff.nodes] - fr_feat_lo) : 0;
    KfCall c;
    for (int pi = 0; pi < n_pairs; pi++) {
        msorb_bow_kf_pair& P = pairs[pi];
        P.nmatches = 0;
        const msorb_kf_store::Entry *A = st->alive(P.kf1), *B = P.kf2 < 0 ? nullptr : st->alive(P.kf2);
        if (!A || (P.kf2 >= 0 && !B) || (P.kf2 < 0) != (frame != nullptr)) {
            set_last_error("search_by_bow_kf: pair " + std::to_string(pi) + ": unknown KeyFrame id, or KeyFrame / frame trains mixed in one call");
            return MSORB_E_INVALID;
        }
        if ((A->n > 0 && (!P.valid1 || !P.match12))) { set_last_error("search_by_bow_kf: null valid1 / match12"); return MSORB_E_INVALID; }
        const KfPair K{A, B, B ? B->n : frame->n, 0, 0, P.match12, P.match21, &P.nmatches};
        if (!(B ? c.add(K) : c.add(K, ff, -fr_feat_lo))) { set_last_error("search_by_bow_kf: node list too long"); return MSORB_E_INVALID; }
    }
    if (c.w.items.empty()) { c.unmatched(); return MSORB_OK; }
    const size_t tot1 = c.tot1, tot2 = c.tot2;
    // [frame desc | frame feat | frame angle | items | posts | valid1 | avail2] in, [match12 | match21 | nmatches] out
    BlockLayout L;
    const size_t o_fd = L.take(fr_rows * 32), o_ff = L.take(fr_feats * 4), o_fa = L.take(fr_rows * 4), o_it = L.take(c.w.item_bytes()),
                 o_po = L.take((size_t)n_pairs * sizeof(PairPost)), o_v1 = L.take(tot1), o_a2 = L.take(tot2);
    L.outputs_begin();
    const size_t o_m = L.take(tot1 * 4), o_m21 = L.take(tot2 * 4), o_nm = L.take((size_t)n_pairs * 4);
    static thread_local ThreadScratch scr(true, 2);
    if (int rc = scr.acquire(st->device, L.end, L.end)) return rc;
    uint8_t *h = scr.h.p, *d = scr.d.p;
    if (fr_rows) std::memcpy(h + o_fd, frame->desc, fr_rows * 32);
    if (fr_feats) std::memcpy(h + o_ff, frame->fv_feat + fr_feat_lo, fr_feats * 4);
    if (fr_rows && frame->angle) std::memcpy(h + o_fa, frame->angle, fr_rows * 4);
    c.w.stage(h + o_it, nullptr, nullptr);
    c.stage_posts(h + o_po);
    for (int pi = 0; pi < n_pairs; pi++) {
        const KfPair& K = c.pairs[pi];
        if (K.A->n) std::memcpy(h + o_v1 + K.m1, pairs[pi].valid1, (size_t)K.A->n);
        if (K.n2) stage_flags(h + o_a2 + K.m2, pairs[pi].avail2, (size_t)K.n2);
    }
    const BlockTrip trip{d, h, L.in_bytes, d + o_m, o_nm - o_m, h + o_m, d + o_m, L.end - o_m};   // match12 and match21 = -1
    if (int rc = round_trip(scr, "search_by_bow_kf", trip, elapsed_ms, [&](hipStream_t s) {
            launch_bow(s, c.w, d + o_it, st->d_desc, frame ? (const uint4*)(d + o_fd) : st->d_desc, d + o_v1, d + o_a2, st->d_feat,
                       frame ? (const int*)(d + o_ff) : st->d_feat, th_low, inclusive ? 1 : 0, nnratio, d + o_m);
            c.launch_histogram(s, d + o_po, st->d_angle, frame ? (const float*)(d + o_fa) : st->d_angle, check_orientation, d + o_m,
                               d + o_m21, d + o_nm);
        })) return rc;
    c.deliver(h + o_m, h + o_m21, h + o_nm);
    return MSORB_OK;
}

extern "C" int msorb_search_for_triangulation_kf(msorb_kf_store* st, msorb_triangulation_kf_pair* pairs, int n_pairs, int coarse,
                                                 int check_orientation, float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (!st || n_pairs < 0 || (n_pairs > 0 && !pairs)) return MSORB_E_INVALID;
    if (n_pairs == 0) return MSORB_OK;
    std::shared_lock<std::shared_mutex> lk(st->mu);
    KfCall c;
    for (int pi = 0; pi < n_pairs; pi++) {
        msorb_triangulation_kf_pair& P = pairs[pi];
        P.nmatches = 0;
        const msorb_kf_store::Entry *A = st->alive(P.kf1), *B = st->alive(P.kf2);
        if (!A || !B) {
            set_last_error("search_for_triangulation_kf: pair " + std::to_string(pi) + ": unknown KeyFrame id");
            return MSORB_E_INVALID;
        }
        if ((A->n > 0 && (!P.valid1 || !P.stereo1 || !P.match12)) || (B->n > 0 && (!P.avail2 || !P.stereo2))) {
            set_last_error("search_for_triangulation_kf: null flag arrays / match12");
            return MSORB_E_INVALID;
        }
        if (!c.add(KfPair{A, B, B->n, 0, 0, P.match12, nullptr, &P.nmatches})) {
            set_last_error("search_for_triangulation_kf: node list too long");
            return MSORB_E_INVALID;
        }
    }
    if (c.w.items.empty()) { c.unmatched(); return MSORB_OK; }
    const size_t tot1 = c.tot1, tot2 = c.tot2;
    // [items | consts | posts | flags1 | flags2] in, [match12 | nmatches] out
    BlockLayout L;
    const size_t o_it = L.take(c.w.item_bytes()), o_c = L.take((size_t)n_pairs * sizeof(TriConst)),
                 o_po = L.take((size_t)n_pairs * sizeof(PairPost)), o_v1 = L.take(tot1), o_a2 = L.take(tot2);
    L.outputs_begin();
    const size_t o_m = L.take(tot1 * 4), o_nm = L.take((size_t)n_pairs * 4);
    static thread_local ThreadScratch scr(true, 2);
    if (int rc = scr.acquire(st->device, L.end, L.end)) return rc;
    uint8_t *h = scr.h.p, *d = scr.d.p;
    c.w.stage(h + o_it, nullptr, nullptr);
    c.stage_posts(h + o_po);
    for (int pi = 0; pi < n_pairs; pi++) {
        const msorb_triangulation_kf_pair& P = pairs[pi];
        const KfPair& K = c.pairs[pi];
        msorb::pack_triangulation_side(K.A->n, nullptr, nullptr, nullptr, P.valid1, P.stereo1, nullptr, nullptr, h + o_v1 + K.m1);
        msorb::pack_triangulation_side(K.n2, nullptr, nullptr, nullptr, P.avail2, P.stereo2, nullptr, nullptr, h + o_a2 + K.m2);
        stage_const(((TriConst*)(h + o_c))[pi], P.F12, P.ep);
    }
    const BlockTrip trip{d, h, L.in_bytes, d + o_m, tot1 * 4, h + o_m, d + o_m, L.end - o_m};
    if (int rc = round_trip(scr, "search_for_triangulation_kf", trip, elapsed_ms, [&](hipStream_t s) {
            launch_triangulation(s, c.w, d + o_it, d + o_c, st->d_desc, st->d_desc, d + o_v1, d + o_a2, st->d_xy, st->d_tr, st->d_feat,
                                 st->d_feat, coarse, d + o_m);
            c.launch_histogram(s, d + o_po, st->d_angle, st->d_angle, check_orientation, d + o_m, nullptr, d + o_nm);
        })) return rc;
    c.deliver(h + o_m, nullptr, h + o_nm);
    return MSORB_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// LocalMapping::CreateNewMapPoints, the loop over the neighbours (LocalMapping.cc:460-731), for resident KeyFrames.
// The reference matches neighbour i+1 against the current KeyFrame's map points AFTER neighbour i's new points were
// added (:722), so the searches cannot share one launch: per neighbour, on one stream, [triangulation_match_kernel over
// that pair's items | pair_histogram_kernel | new_points_kernel], all reading ONE working flag array of KeyFrame 1 in
// the call's scratch, in which new_points_kernel clears the "visited" bit of every feature that got a point.
// ------------------------------------------------------------------------------------------------------------------
namespace {
struct NpSide {   // one KeyFrame of the call
    msorb::NpCam cam;
    int row0;     // its first row in the store's arrays
    int m;        // its first entry in the per-call arrays (flags, u_right, depth)
    int lvl;      // its first entry in the per-call table of level scale factors
    int n;
};

// One thread per feature of KeyFrame 1: a matched one runs LocalMapping.cc:578-712 for its pair (new_points_device.h).
// flag byte: bit 0 visited / available, bit 1 stereo, bits 2..7 the keypoint's octave.
__global__ __launch_bounds__(256) void new_points_kernel(const NpSide* __restrict__ sides, int k2, const float* __restrict__ lvl_scale,
                                                         uint8_t* __restrict__ flags, const float* __restrict__ u_right,
                                                         const float* __restrict__ depth, const float2* __restrict__ xy,
                                                         const float4* __restrict__ tr, const int* __restrict__ match12, int inertial,
                                                         float th_far, float ratio_factor, uint8_t* __restrict__ status,
                                                         float* __restrict__ x3d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n1 = sides[0].n, n2 = sides[k2].n;
    if (i >= n1) return;
    const int i2 = match12[i];
    uint8_t st = msorb::kNpNone;
    float X[3] = {0.0f, 0.0f, 0.0f};
    if (i2 >= 0 && i2 < n2) {
        const NpSide& S1 = sides[0];
        const NpSide& S2 = sides[k2];
        const uint8_t fl1 = flags[S1.m + i], fl2 = flags[S2.m + i2];
        const float2 p1 = xy[S1.row0 + i];
        const float4 t2 = tr[S2.row0 + i2];
        const msorb::NpFeature f1{p1.x, p1.y, u_right[S1.m + i], depth[S1.m + i], tr[S1.row0 + i].w, lvl_scale[S1.lvl + (fl1 >> 2)]};
        const msorb::NpFeature f2{t2.x, t2.y, u_right[S2.m + i2], depth[S2.m + i2], t2.w, lvl_scale[S2.lvl + (fl2 >> 2)]};
        st = msorb::new_point_pair(S1.cam, S2.cam, f1, f2, inertial, th_far, ratio_factor, X);
        if (st >= msorb::kNpTriangulated && st <= msorb::kNpStereo2) flags[S1.m + i] = fl1 & ~1u;   // :722: no query of the next neighbour
        else X[0] = X[1] = X[2] = 0.0f;
    }
    status[i] = st;
    x3d[3 * i] = X[0];
    x3d[3 * i + 1] = X[1];
    x3d[3 * i + 2] = X[2];
}

bool np_geometry_ok(const msorb_new_points_geometry& g, int n) { return n == 0 || (g.u_right && g.depth); }
void np_stage_side(NpSide& S, const msorb_new_points_geometry& g, const msorb_kf_store::Entry& E, int m, int lvl, const uint8_t* on,
                   uint8_t* flags, float* ur, float* depth, float* lvl_scale) {
    std::memcpy(S.cam.T, g.Tcw, sizeof(g.Tcw));
    std::memcpy(S.cam.Ow, g.Ow, sizeof(g.Ow));
    S.cam.fx = g.fx; S.cam.fy = g.fy; S.cam.cx = g.cx; S.cam.cy = g.cy;
    S.cam.invfx = g.invfx; S.cam.invfy = g.invfy; S.cam.mb = g.mb; S.cam.mbf = g.mbf;
    S.row0 = E.row0; S.m = m; S.lvl = lvl; S.n = E.n;
    for (int i = 0; i < E.n; i++) flags[m + i] = (uint8_t)((on[i] ? 1 : 0) | (g.u_right[i] >= 0.0f ? 2 : 0) | (E.octave[i] << 2));
    if (E.n) { std::memcpy(ur + m, g.u_right, (size_t)E.n * 4); std::memcpy(depth + m, g.depth, (size_t)E.n * 4); }
    std::memcpy(lvl_scale + lvl, E.scale.data(), E.scale.size() * 4);
}
thread_local float g_np_stage_ms[3] = {0, 0, 0};
bool np_stage_events() {
    static const bool on = [] { const char* e = getenv("MSORB_NEW_POINTS_STAGES"); return e && e[0] == '1'; }();
    return on;
}
}  // namespace

extern "C" int msorb_create_new_map_points_stage_ms(float ms[3]) {
    if (!ms) return MSORB_E_INVALID;
    std::memcpy(ms, g_np_stage_ms, sizeof(g_np_stage_ms));
    return MSORB_OK;
}

extern "C" int msorb_create_new_map_points_kf(msorb_kf_store* st, const msorb_new_points_call* call, msorb_new_points_neighbour* nb,
                                              int n_nb, float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (!st || !call || n_nb < 0 || (n_nb > 0 && !nb)) return MSORB_E_INVALID;
    std::shared_lock<std::shared_mutex> lk(st->mu);
    const msorb_kf_store::Entry* A = st->alive(call->kf1);
    if (!A || (A->n > 0 && !call->valid1) || !np_geometry_ok(call->g1, A->n) || A->scale.size() > 64) {
        set_last_error("create_new_map_points_kf: unknown kf1 / null valid1, u_right or depth / more than 64 levels");
        return MSORB_E_INVALID;
    }
    const int n1 = A->n;
    NodeWork w;
    std::vector<const msorb_kf_store::Entry*> B((size_t)n_nb);
    std::vector<int> item0((size_t)n_nb + 1, 0), m2((size_t)n_nb), lvl((size_t)n_nb);
    size_t tot = (size_t)n1, tot_lvl = A->scale.size();
    for (int k = 0; k < n_nb; k++) {
        msorb_new_points_neighbour& N = nb[k];
        N.nmatches = 0;
        N.n_created = 0;
        B[k] = N.kf2 == call->kf1 ? nullptr : st->alive(N.kf2);
        bool ok = B[k] != nullptr;
        for (int j = 0; ok && j < k; j++) ok = nb[j].kf2 != N.kf2;
        ok = ok && (B[k]->n == 0 || N.avail2) && np_geometry_ok(N.g2, B[k]->n) && (n1 == 0 || (N.match12 && N.status && N.x3D)) &&
             B[k]->scale.size() <= 64;
        if (!ok) {
            set_last_error("create_new_map_points_kf: neighbour " + std::to_string(k) +
                           ": unknown kf2 / kf2 == kf1 / kf2 listed twice / null array / more than 64 levels");
            return MSORB_E_INVALID;
        }
        m2[k] = (int)tot;
        lvl[k] = (int)tot_lvl;
        tot += (size_t)B[k]->n;
        tot_lvl += B[k]->scale.size();
        if (tot > (size_t)INT32_MAX / 16 || (size_t)(k + 1) * (size_t)n1 > (size_t)INT32_MAX / 16) return MSORB_E_INVALID;
        if (!w.add(A->fv(), B[k]->fv(), k, A->row0, B[k]->row0, 0, m2[k], A->feat0, B[k]->feat0)) {
            set_last_error("create_new_map_points_kf: node list too long");
            return MSORB_E_INVALID;
        }
        item0[k + 1] = (int)w.items.size();
    }
    for (int k = 0; k < n_nb && n1; k++) {
        std::fill_n(nb[k].match12, n1, -1);
        std::memset(nb[k].status, 0, (size_t)n1);
        std::memset(nb[k].x3D, 0, (size_t)n1 * 12);
    }
    if (w.items.empty() || n1 == 0) return MSORB_OK;
    const size_t K = (size_t)n_nb, kn1 = K * (size_t)n1;
    // [items | consts | posts | sides | level scales | u_right | depth | flags] in, [match12 | nmatches | x3D | status] out
    BlockLayout L;
    const size_t o_it = L.take(w.item_bytes()), o_c = L.take(K * sizeof(TriConst)), o_po = L.take(K * sizeof(PairPost)),
                 o_sd = L.take((K + 1) * sizeof(NpSide)), o_lv = L.take(tot_lvl * 4), o_ur = L.take(tot * 4), o_dp = L.take(tot * 4),
                 o_fl = L.take(tot);
    L.outputs_begin();
    const size_t o_m = L.take(kn1 * 4), o_nm = L.take(K * 4), o_x = L.take(kn1 * 12), o_st = L.take(kn1);
    static thread_local ThreadScratch scr(true, 2);
    if (int rc = scr.acquire(st->device, L.end, L.end)) return rc;
    uint8_t *h = scr.h.p, *d = scr.d.p;
    w.stage(h + o_it, nullptr, nullptr);
    NpSide* sides = (NpSide*)(h + o_sd);
    np_stage_side(sides[0], call->g1, *A, 0, 0, call->valid1, h + o_fl, (float*)(h + o_ur), (float*)(h + o_dp), (float*)(h + o_lv));
    for (size_t k = 0; k < K; k++) {
        np_stage_side(sides[k + 1], nb[k].g2, *B[k], m2[k], lvl[k], nb[k].avail2, h + o_fl, (float*)(h + o_ur), (float*)(h + o_dp),
                      (float*)(h + o_lv));
        stage_const(((TriConst*)(h + o_c))[k], nb[k].F12, nb[k].ep);
        ((PairPost*)(h + o_po))[k] = PairPost{(int)(k * (size_t)n1), n1, 0, B[k]->n, A->row0, B[k]->row0};
    }
    const float ratio_factor = 1.5f * (A->scale.size() > 1 ? A->scale[1] : 1.0f);   // 1.5f * mfScaleFactor (:454)
    const bool stages = elapsed_ms && np_stage_events();
    std::vector<hipEvent_t> ev;
    if (stages) {
        ev.assign(3 * K + 1, nullptr);
        for (hipEvent_t& e : ev)
            if (hipEventCreate(&e) != hipSuccess) { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); return MSORB_E_HIP; }
    }
    size_t e = 0;   // events recorded
    const BlockTrip trip{d, h, L.in_bytes, d + o_m, kn1 * 4, h + o_m, d + o_m, L.end - o_m};
    const int rc = round_trip(scr, "create_new_map_points_kf", trip, elapsed_ms, [&](hipStream_t s) {
        (void)hipMemsetAsync(d + o_nm, 0, L.end - o_nm, s);   // nmatches, x3D and status of the neighbours that launch nothing
        if (stages) (void)hipEventRecord(ev[e++], s);
        for (size_t k = 0; k < K; k++) {
            const int cnt = item0[k + 1] - item0[k];
            if (cnt == 0) continue;
            int* match12 = (int*)(d + o_m) + k * (size_t)n1;
            hipLaunchKernelGGL(triangulation_match_kernel, dim3((unsigned)cnt), dim3(64), w.lds(), s,
                               (const BowItem*)(d + o_it) + item0[k], (const TriConst*)(d + o_c), st->d_desc, st->d_desc, d + o_fl, d + o_fl,
                               st->d_xy, st->d_tr, st->d_feat, st->d_feat, call->coarse, match12);
            if (stages) (void)hipEventRecord(ev[e++], s);
            hipLaunchKernelGGL(pair_histogram_kernel, dim3(1), dim3(256), 0, s, (const PairPost*)(d + o_po) + k, st->d_angle, st->d_angle,
                               call->check_orientation, (int*)(d + o_m), (int*)nullptr, (int*)(d + o_nm) + k);
            if (stages) (void)hipEventRecord(ev[e++], s);
            hipLaunchKernelGGL(new_points_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s, (const NpSide*)(d + o_sd), (int)k + 1,
                               (const float*)(d + o_lv), d + o_fl, (const float*)(d + o_ur), (const float*)(d + o_dp), st->d_xy, st->d_tr,
                               match12, call->inertial, call->th_far, ratio_factor, d + o_st + k * (size_t)n1,
                               (float*)(d + o_x) + 3 * k * (size_t)n1);
            if (stages) (void)hipEventRecord(ev[e++], s);
        }
    });
    if (stages && rc == MSORB_OK) {
        g_np_stage_ms[0] = g_np_stage_ms[1] = g_np_stage_ms[2] = 0;
        for (size_t i = 1; i < e; i++) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev[i - 1], ev[i]) == hipSuccess) g_np_stage_ms[(i - 1) % 3] += ms;
        }
    }
    if (stages)   // (a failed trip has released the scratch, the device is still current)
        for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
    if (rc) return rc;
    for (size_t k = 0; k < K; k++) {
        msorb_new_points_neighbour& N = nb[k];
        std::memcpy(N.match12, h + o_m + k * (size_t)n1 * 4, (size_t)n1 * 4);
        std::memcpy(N.x3D, h + o_x + k * (size_t)n1 * 12, (size_t)n1 * 12);
        std::memcpy(N.status, h + o_st + k * (size_t)n1, (size_t)n1);
        N.nmatches = ((const int*)(h + o_nm))[k];
        for (int i = 0; i < n1; i++) N.n_created += N.status[i] >= MSORB_NP_TRIANGULATED && N.status[i] <= MSORB_NP_STEREO2;
    }
    return MSORB_OK;
}
