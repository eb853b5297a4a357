// The claim replay of the SearchByProjection forms (ORBmatcher.cc:88-90,129), free of HIP.  SearchByProjection assigns
// F.mvpMapPoints[bestIdx] inside its loop, and later queries skip keypoints that hold a map point with Observations() > 0.  The
// device ranks, for every query at once, the kTopK best candidates against an occupancy SNAPSHOT; the host replays the accept
// rule in query order, dropping candidates claimed since the snapshot.  A query whose list can no longer be trusted — exhausted
// by claims, or a keypoint inside its window was freed since (a point without observations overwrote an occupied keypoint) —
// asks for a new round: the snapshot is refreshed and the lists recomputed from that query on.  The result is always what the
// reference's sequential loop gives.
//   Beside the rule (ClaimSide, replay_claims) this header holds what the rule is replayed WITH for SearchByProjection(F, MapPoints):
// the accept decision and the two-camera interleaving of the passes, so that the CPU test (tests/claim_replay_main.cc) runs the
// loop the library ships.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "window_query.h"

namespace msorb {

// One frame's side of a replay: its occupancy against the snapshot its lists were computed for.
struct ClaimSide {
    const msorb_keypoint* kps = nullptr;   // the frame's keypoints [N]
    int N = 0;
    const WinQuery* q = nullptr;           // nullptr: the queries were built on the device, their windows are unknown here
    const uint8_t* flags = nullptr;        // kQValid / kQSkipOccupied per query; nullptr: taken from q
    const TopK* topk = nullptr;            // the device's lists, refilled from `from` on by every round
    uint8_t* occ = nullptr;                // the live occupancy [N]
    std::vector<uint8_t> snap;             // the occupancy the lists were computed against
    std::vector<int8_t> diff;              // occupancy now vs snap: +1 claimed since, -1 freed since
    std::vector<int> freed;                // keypoints freed since the round (entries whose diff is no longer negative were claimed again)
    int n_freed = 0, fresh_from = 0, rounds = 0;
    bool pristine = true;   // no occupancy change since the last round: only then is the list of query `fresh_from` exact as it stands.
                            // (With two cameras the OTHER camera's pass of the same map point can change this side between its round and
                            // its first query: a left match of a point without observations frees the right partner it overwrites,
                            // ORBmatcher.cc:130-134.  With one camera the first query of a round always finds the side pristine.)

    uint8_t flag(int qi) const { return flags ? flags[qi] : q[qi].flags; }

    void begin_round(int from) {   // the lists of queries [from, ...) have just been computed against occ
        snap.assign(occ, occ + N);
        diff.assign(N, 0);
        freed.clear();
        n_freed = 0;
        fresh_from = from;
        pristine = true;
        rounds++;
    }
    void set_occ(int idx, int v) {
        pristine = false;
        occ[idx] = (uint8_t)v;
        const int8_t d = (int8_t)((int)occ[idx] - (int)snap[idx]);
        if (diff[idx] < 0) n_freed--;
        diff[idx] = d;
        if (d < 0) { n_freed++; freed.push_back(idx); }
    }
    // a keypoint that was occupied at the round and is free now is missing from the lists of exactly those queries whose window
    // (box and level band as window_topk_kernel tests them; its mvuRight test can only drop more) holds it: only they need a new round
    bool window_holds_a_freed_keypoint(const WinQuery& w) const {
        for (int idx : freed) {
            if (diff[idx] >= 0) continue;
            const msorb_keypoint& kp = kps[idx];
            if (kp.octave < w.min_level || (w.max_level >= 0 && kp.octave > w.max_level)) continue;
            if (fabsf(kp.x - w.x) < w.r && fabsf(kp.y - w.y) < w.r) return true;
        }
        return false;
    }
    // the exact candidate prefix of query qi (>= need entries unless the true candidate set is smaller); false: the list cannot be
    // trusted any more (exhausted by claims, or a keypoint was freed): the side needs a new round from qi
    bool prefix(int qi, int need, int* idx, int* dist, int* n_out) const {
        *n_out = 0;
        if (N <= 0) return true;
        const bool skip = flag(qi) & kQSkipOccupied;
        const bool stale = qi > fresh_from || !pristine;   // claims may lie between the round and this query
        if (skip && n_freed > 0 && stale && (!q || window_holds_a_freed_keypoint(q[qi]))) return false;
        const TopK& t = topk[qi];
        int n = 0, n_dev = 0;
        for (int k = 0; k < kTopK; k++) {
            if (t.idx[k] < 0) break;
            n_dev++;
            if (skip && diff[t.idx[k]] > 0) continue;
            idx[n] = t.idx[k]; dist[n] = t.dist[k]; n++;
        }
        if (n < need && n < n_dev && n_dev == kTopK && stale) return false;
        *n_out = n;
        return true;
    }
};

// One side, queries [0, M) in order.  round(from) refills S.topk[from, M) against S.occ as it stands (0, or a negative error that
// ends the replay); ready: the caller has run round 0 already.  accept(qi, idx, dist, n, &new_occ) gets the query's exact candidate
// prefix and returns the keypoint it assigned (or -1) and that keypoint's new occupancy.  Returns the number of rounds (S.rounds).
template <typename Round, typename Accept>
int replay_claims(ClaimSide& S, int M, int need, bool ready, Round round, Accept accept) {
    if (M <= 0 || S.N <= 0) return 0;   // no queries / no keypoints: no match
    for (int q0 = 0;;) {
        if (!(ready && S.rounds == 0))
            if (const int rc = round(q0)) return rc;
        S.begin_round(q0);
        int qi = q0;
        for (; qi < M; qi++) {
            if (!(S.flag(qi) & kQValid)) continue;
            int idx[kTopK], dist[kTopK], n;
            if (!S.prefix(qi, need, idx, dist, &n)) break;
            int new_occ = 0;
            const int assigned = accept(qi, idx, dist, n, &new_occ);
            if (assigned >= 0) S.set_occ(assigned, new_occ);
        }
        if (qi == M) return S.rounds;
        q0 = qi;
    }
}

// The accept decision of SearchByProjection(F, MapPoints) on a candidate prefix (best, second), ORBmatcher.cc:122-141: the
// keypoint, kNoMatch, or kRatioFailed (best and second on the same level and too close: :125-126, where the loop `continue`s).
// (A NaN nnratio fails both comparisons: no match, as in the reference's left pass.)
constexpr int kNoMatch = -1, kRatioFailed = -2;
inline int accept_best_of_two(const msorb_keypoint* kps, const int* idx, const int* dist, int n, float nnratio) {
    if (n == 0) return kNoMatch;
    const int bestDist = dist[0], bestIdx = idx[0];
    const int bestLevel = kps[bestIdx].octave;
    const int bestDist2 = n > 1 ? dist[1] : 256;
    const int bestLevel2 = n > 1 ? kps[idx[1]].octave : -1;
    if (bestDist > kThHigh) return kNoMatch;
    if (bestLevel == bestLevel2 && bestDist > nnratio * bestDist2) return kRatioFailed;
    if (bestLevel != bestLevel2 || bestDist <= nnratio * bestDist2) return bestIdx;
    return kNoMatch;
}

// Two cameras: SearchByProjection(F, MapPoints) on a frame with F.Nleft != -1 (ORBmatcher.cc:43-213).  Per map point a LEFT pass
// over L and then a RIGHT pass over R, both with the accept rule above.  What couples the sides, replayed here in map-point order:
//   * a left match also claims the right keypoint it is stereo-matched with (mvLeftToRightMatch, :130-134), a right match the left
//     one (mvRightToLeftMatch, :196-200): the occupancy each LATER map point sees on either side;
//   * a left pass that fails its ratio test `continue`s the map-point loop (:125-126): the right pass of that point is skipped.
// frame_mp is F.mvpMapPoints [L.N + R.N]; a claim of map point i leaves the occupancy obs[i] > 0.  Each side asks for its own new
// rounds (round_left / round_right as in replay_claims); the other side goes on from where it stopped.  Returns 0 or the error of a
// round; the rounds are L.rounds / R.rounds.
template <typename RoundL, typename RoundR>
int replay_claims_two_cameras(ClaimSide& L, ClaimSide& R, int M, const int* obs, const int* left_to_right, const int* right_to_left,
                              int* frame_mp, float nnratio, RoundL round_left, RoundR round_right, int* nmatches) {
    const int NL = L.N;
    int nm = 0, nextL = 0, nextR = 0;
    bool needL = true, needR = true;
    std::vector<uint8_t> skip_right(M > 0 ? M : 0, 0);   // the left pass of the point `continue`d the loop
    while (needL || needR) {
        if (needL) {
            if (const int rc = round_left(nextL)) return rc;
            L.begin_round(nextL);
        }
        if (needR) {
            if (const int rc = round_right(nextR)) return rc;
            R.begin_round(nextR);
        }
        needL = needR = false;
        for (int i = nextL < nextR ? nextL : nextR; i < M; i++) {
            int idx[kTopK], dist[kTopK], n = 0;
            if (i >= nextL) {
                if (L.flag(i) & kQValid) {
                    if (!L.prefix(i, 2, idx, dist, &n)) { needL = true; break; }
                    const int b = accept_best_of_two(L.kps, idx, dist, n, nnratio);
                    if (b == kRatioFailed) skip_right[i] = 1;
                    if (b >= 0) {
                        frame_mp[b] = i; nm++;
                        L.set_occ(b, obs[i] > 0);
                        if (left_to_right[b] != -1) {                    // :130-134
                            frame_mp[NL + left_to_right[b]] = i; nm++;
                            R.set_occ(left_to_right[b], obs[i] > 0);
                        }
                    }
                }
                nextL = i + 1;
            }
            if (i >= nextR) {
                if (!skip_right[i] && (R.flag(i) & kQValid)) {
                    if (!R.prefix(i, 2, idx, dist, &n)) { needR = true; break; }
                    const int b = accept_best_of_two(R.kps, idx, dist, n, nnratio);
                    if (b >= 0) {
                        if (right_to_left[b] != -1) {                    // :196-200
                            frame_mp[right_to_left[b]] = i; nm++;
                            L.set_occ(right_to_left[b], obs[i] > 0);
                        }
                        frame_mp[NL + b] = i; nm++;
                        R.set_occ(b, obs[i] > 0);
                    }
                }
                nextR = i + 1;
            }
        }
    }
    *nmatches = nm;
    return 0;
}

}  // namespace msorb
