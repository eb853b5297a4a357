// The claim replay of ms-slam_amd/csrc/claim_replay.h on the CPU, against the reference's sequential loop.  This program plays the
// device itself: `device_round` ranks, per query, the first kTopK candidates (box test, level band, skip-if-occupied-at-the-snapshot)
// in the fixed order (distance, keypoint index); the brute force takes the queries in order, scans the keypoints against the LIVE
// occupancy with strict `<` for best / second and applies the accept rule.  Matches, final occupancy and match count must be equal
// on every drawn scene.  Forms: one side with the level / ratio rule (need 2), one side with the distance threshold (need 1), two
// cameras with partner claims (the shipped replay_claims_two_cameras) — each also with queries "built on the device" (q == nullptr on
// one side: flags only, windows unknown to the replay).
//
// Coverage, counted per form in scenes: (a) a new round because a list was exhausted by claims, (b) a new round because a keypoint
// was freed (inside the query's window where the windows are known), (c) two cameras: a side changed by the other camera before
// its first query after a round.  The program fails unless each class occurs in at least 10 % of the form's scenes.  Every new
// round must also have been NEEDED (struct Why): asking too often is invisible in the matches.
//   (c) can only happen to the right camera at map point 0: a side that asked for a round at point i examines point i first, before
// the other side runs again; only the very first rounds are taken for both sides at once, and the left pass of point 0 precedes the
// right one.  It is counted in the brute force: the left pass of point 0 claims a keypoint with a partner and the right pass runs.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "claim_replay.h"
#include "window_query.h"

using namespace msorb;

#define CHECK(c)                                                                                     \
    do {                                                                                             \
        if (!(c)) { std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, g_where); std::exit(1); } \
    } while (0)
static char g_where[128] = "";

struct Rng {   // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    float unit() { return (float)(next() >> 40) / (float)(1 << 24); }
    bool chance(float p) { return unit() < p; }
};

static int distance(uint64_t a, uint64_t b) { return 3 * __builtin_popcountll(a ^ b); }   // a few distinct values: ties, ratio failures
static uint64_t flip(Rng& g, uint64_t d, int max_flips) {
    for (int k = g.below(max_flips + 1); k > 0; k--) d ^= 1ull << g.below(64);
    return d;
}

struct Camera {
    int N = 0;
    std::vector<msorb_keypoint> kps;
    std::vector<uint64_t> desc;
    std::vector<uint8_t> occ0;     // occupancy before the search
    std::vector<WinQuery> q;       // [M]
};
struct Scene {
    int M = 0;
    Camera cam[2];
    std::vector<uint64_t> qdesc;
    std::vector<int> obs, l2r, r2l;
};

static bool in_window(const msorb_keypoint& kp, const WinQuery& w) {
    if (kp.octave < w.min_level || (w.max_level >= 0 && kp.octave > w.max_level)) return false;
    return std::fabs(kp.x - w.x) < w.r && std::fabs(kp.y - w.y) < w.r;
}

// keypoints packed into a 40 x 20 pixel patch (two by three grid cells of a KITTI frame), three levels, five descriptor families
static Scene draw_scene(uint64_t seed, int index, bool two_cameras) {
    Rng g{seed};
    Scene sc;
    const int n_cam = two_cameras ? 2 : 1;
    sc.M = index % 30 == 7 ? 0 : g.below(601);
    const float no_obs = 0.10f + 0.20f * g.unit(), no_skip = 0.05f + 0.15f * g.unit();
    uint64_t family[5];
    for (uint64_t& f : family) f = g.next();
    for (int c = 0; c < n_cam; c++) {
        Camera& cam = sc.cam[c];
        cam.N = (index % 25 == 3 + c || index % 50 == 11) ? 0 : g.below(301);
        cam.kps.assign(cam.N, msorb_keypoint{});
        cam.desc.resize(cam.N);
        cam.occ0.resize(cam.N);
        for (int i = 0; i < cam.N; i++) {
            cam.kps[i].x = 100.0f + 40.0f * g.unit(); cam.kps[i].y = 50.0f + 20.0f * g.unit();
            cam.kps[i].octave = g.below(3);
            cam.desc[i] = flip(g, family[g.below(5)], 2);
            cam.occ0[i] = g.chance(0.2f);
        }
    }
    const int NL = sc.cam[0].N, NR = sc.cam[1].N;
    sc.l2r.assign(NL, -1); sc.r2l.assign(NR, -1);
    if (two_cameras)   // stereo partners: right keypoint j re-detects left keypoint r2l[j]
        for (int i = 0, j = 0; i < NL && j < NR; i++) {
            if (!g.chance(0.6f)) continue;
            sc.l2r[i] = j; sc.r2l[j] = i;
            sc.cam[1].desc[j] = flip(g, sc.cam[0].desc[i], 2);
            sc.cam[1].kps[j].octave = sc.cam[0].kps[i].octave;
            j += 1 + g.below(2);
        }
    sc.qdesc.resize(sc.M); sc.obs.resize(sc.M);
    for (int c = 0; c < n_cam; c++) sc.cam[c].q.assign(sc.M, WinQuery{});
    for (int i = 0; i < sc.M; i++) {
        sc.obs[i] = g.chance(no_obs) ? 0 : 1 + g.below(5);
        const int src = NL ? g.below(NL) : -1;
        // (two cameras: half of the scenes start with a point that copies a left keypoint: its left match claims the right partner)
        const bool copy = i == 0 && two_cameras && (index & 1);
        sc.qdesc[i] = src >= 0 && (copy || g.chance(0.7f)) ? flip(g, sc.cam[0].desc[src], copy ? 0 : 3) : (NR && g.chance(0.5f) ? sc.cam[1].desc[g.below(NR)] : g.next());
        for (int c = 0; c < n_cam; c++) {
            const Camera& cam = sc.cam[c];
            int at = c == 0 ? src : (src >= 0 && sc.l2r[src] >= 0 && g.chance(0.8f) ? sc.l2r[src] : (cam.N ? g.below(cam.N) : -1));
            WinQuery& w = sc.cam[c].q[i];
            const float cx = at >= 0 ? cam.kps[at].x : 120.0f, cy = at >= 0 ? cam.kps[at].y : 60.0f;
            w.x = cx + (copy ? 0.0f : 4.0f * (g.unit() - 0.5f)); w.y = cy + (copy ? 0.0f : 4.0f * (g.unit() - 0.5f));
            const int level = (at >= 0 ? cam.kps[at].octave : 1) + (copy ? 0 : g.below(2));
            w.r = (g.chance(0.5f) ? 2.5f : 4.0f) * (1.0f + 0.5f * (float)level);
            w.min_level = (int16_t)(level - 1); w.max_level = (int16_t)(g.chance(0.1f) ? -1 : level);
            const bool skip = c == 1 || !g.chance(no_skip);   // the right pass has no mbSparsified bypass
            w.flags = (copy || g.chance(0.85f)) ? (uint8_t)(kQValid | (skip ? kQSkipOccupied : 0)) : 0;
        }
    }
    return sc;
}

// ---- the stand-in for the device ----
struct Device {
    const Camera* cam;
    std::vector<std::vector<std::pair<int, int>>> cand;   // per query: (distance, keypoint) inside the window, ordered
    std::vector<TopK> lists;
    std::vector<uint8_t> snap;                            // the occupancy of the last round
    Device(const Camera& c, const std::vector<uint64_t>& qdesc) : cam(&c), cand(qdesc.size()), lists(qdesc.size()) {
        for (size_t qi = 0; qi < qdesc.size(); qi++) {
            if (!(c.q[qi].flags & kQValid)) continue;
            for (int k = 0; k < c.N; k++)
                if (in_window(c.kps[k], c.q[qi])) cand[qi].push_back({distance(qdesc[qi], c.desc[k]), k});
            std::sort(cand[qi].begin(), cand[qi].end());
        }
    }
    void round(const uint8_t* occ, int from) {   // lists of queries [from, M) against the occupancy as it is now
        snap.assign(occ, occ + cam->N);
        for (size_t qi = (size_t)from; qi < cand.size(); qi++) {
            TopK& t = lists[qi];
            int n = 0;
            const bool skip = cam->q[qi].flags & kQSkipOccupied;
            for (const auto& c : cand[qi]) {
                if (skip && occ[c.second]) continue;
                t.dist[n] = c.first; t.idx[n] = c.second;
                if (++n == kTopK) break;
            }
            for (; n < kTopK; n++) { t.idx[n] = -1; t.dist[n] = 256; }
        }
    }
};

// ---- the reference's loop ----
struct Best {
    int idx = -1, dist = 256, level = -1, dist2 = 256, level2 = -1;
};
static Best scan(const Camera& cam, const WinQuery& w, uint64_t d, const std::vector<uint8_t>& occ) {
    Best b;
    for (int k = 0; k < cam.N; k++) {
        if (!in_window(cam.kps[k], w)) continue;
        if ((w.flags & kQSkipOccupied) && occ[k]) continue;
        const int dist = distance(d, cam.desc[k]);
        if (dist < b.dist) { b.dist2 = b.dist; b.level2 = b.level; b.dist = dist; b.level = cam.kps[k].octave; b.idx = k; }
        else if (dist < b.dist2) { b.dist2 = dist; b.level2 = cam.kps[k].octave; }
    }
    return b;
}
struct Result {
    std::vector<int> mp;          // F.mvpMapPoints: [NL + NR]
    std::vector<uint8_t> occ[2];
    int nmatches = 0;
    bool operator==(const Result& o) const { return mp == o.mp && occ[0] == o.occ[0] && occ[1] == o.occ[1] && nmatches == o.nmatches; }
};
static Result start(const Scene& sc) {
    Result r;
    r.mp.assign(sc.cam[0].N + sc.cam[1].N, -1);
    r.occ[0] = sc.cam[0].occ0; r.occ[1] = sc.cam[1].occ0;
    return r;
}
static const float kRatio = 0.8f;
static const int kThreshold = 60;   // need 1: between the distances inside a descriptor family and across families

static Result brute_one_side(const Scene& sc, int need) {
    Result r = start(sc);
    const Camera& cam = sc.cam[0];
    for (int i = 0; i < sc.M; i++) {
        if (!(cam.q[i].flags & kQValid)) continue;
        const Best b = scan(cam, cam.q[i], sc.qdesc[i], r.occ[0]);
        bool take;
        if (need == 2) take = b.dist <= kThHigh && !(b.level == b.level2 && b.dist > kRatio * b.dist2);   // ORBmatcher.cc:122-141
        else take = b.idx >= 0 && b.dist <= kThreshold;
        if (take) { r.mp[b.idx] = i; r.nmatches++; r.occ[0][b.idx] = sc.obs[i] > 0; }
    }
    return r;
}
static Result brute_two_cameras(const Scene& sc, bool* right_changed_before_its_first_query) {
    Result r = start(sc);
    const int NL = sc.cam[0].N;
    *right_changed_before_its_first_query = false;
    for (int i = 0; i < sc.M; i++) {
        bool left_claimed_a_partner = false;
        if (sc.cam[0].q[i].flags & kQValid) {
            const Best b = scan(sc.cam[0], sc.cam[0].q[i], sc.qdesc[i], r.occ[0]);
            if (b.dist <= kThHigh) {
                if (b.level == b.level2 && b.dist > kRatio * b.dist2) continue;   // :125-126
                r.mp[b.idx] = i; r.nmatches++; r.occ[0][b.idx] = sc.obs[i] > 0;
                if (sc.l2r[b.idx] != -1) {
                    r.mp[NL + sc.l2r[b.idx]] = i; r.nmatches++; r.occ[1][sc.l2r[b.idx]] = sc.obs[i] > 0;
                    left_claimed_a_partner = true;
                }
            }
        }
        if (sc.cam[1].q[i].flags & kQValid) {
            if (i == 0 && left_claimed_a_partner && sc.cam[1].N > 0) *right_changed_before_its_first_query = true;
            const Best b = scan(sc.cam[1], sc.cam[1].q[i], sc.qdesc[i], r.occ[1]);
            if (b.dist <= kThHigh) {
                if (b.level == b.level2 && b.dist > kRatio * b.dist2) continue;   // :195-196
                if (sc.r2l[b.idx] != -1) { r.mp[sc.r2l[b.idx]] = i; r.nmatches++; r.occ[0][sc.r2l[b.idx]] = sc.obs[i] > 0; }
                r.mp[NL + b.idx] = i; r.nmatches++; r.occ[1][b.idx] = sc.obs[i] > 0;
            }
        }
    }
    return r;
}

// ---- the replay under test ----
struct Coverage {
    int scenes = 0, exhausted = 0, freed = 0, changed = 0;
};
// Why a side asked for a new round at query `from`, worked out from the device's own snapshot and the live occupancy, not from the
// side's bookkeeping — and that it HAD to ask: a keypoint occupied at the snapshot and free now lies in the query's window (anywhere
// in the frame where the windows are unknown to the replay), or the stale list is full and too few of its entries are still free.
// A replay that asks more often than that still gives the right matches; only this check sees it.
struct Why {
    bool exhausted = false, freed = false;
    void note(const ClaimSide& S, const Device& dev, int from, int need) {
        if (S.rounds == 0) return;
        const Camera& cam = *dev.cam;
        const WinQuery& w = cam.q[from];
        const bool skip = w.flags & kQSkipOccupied;
        bool f = false;
        for (int k = 0; k < cam.N && skip && !f; k++) f = dev.snap[k] && !S.occ[k] && (!S.q || in_window(cam.kps[k], w));
        int listed = 0, kept = 0;
        for (int k = 0; k < kTopK && dev.lists[from].idx[k] >= 0; k++) {
            listed++;
            kept += !(skip && S.occ[dev.lists[from].idx[k]]);
        }
        const bool e = listed == kTopK && kept < listed && kept < need;
        CHECK(f || e);
        (f ? freed : exhausted) = true;
    }
};
static ClaimSide side_of(const Camera& cam, const Device& dev, std::vector<uint8_t>& occ, std::vector<uint8_t>& flags, bool device_built) {
    ClaimSide S;
    S.kps = cam.kps.data(); S.N = cam.N; S.topk = dev.lists.data(); S.occ = occ.data();
    flags.resize(cam.q.size());
    for (size_t i = 0; i < cam.q.size(); i++) flags[i] = cam.q[i].flags;
    if (device_built) S.flags = flags.data();   // windows unknown
    else S.q = cam.q.data();                     // flags taken from the queries
    return S;
}

static void one_side(const Scene& sc, int need, bool device_built, bool ready, Coverage& cov) {
    const Result want = brute_one_side(sc, need);
    Result got = start(sc);
    const Camera& cam = sc.cam[0];
    Device dev(cam, sc.qdesc);
    std::vector<uint8_t> flags;
    ClaimSide S = side_of(cam, dev, got.occ[0], flags, device_built);
    Why why;
    if (ready) dev.round(S.occ, 0);   // round 0 run by the caller
    int rounds_taken = ready ? 1 : 0;
    const int rounds = replay_claims(S, sc.M, need, ready,
        [&](int from) { why.note(S, dev, from, need); dev.round(S.occ, from); rounds_taken++; return 0; },
        [&](int qi, const int* idx, const int* dist, int n, int* new_occ) {
            int b;
            if (need == 2) b = accept_best_of_two(cam.kps.data(), idx, dist, n, kRatio);
            else b = n > 0 && dist[0] <= kThreshold ? idx[0] : -1;
            if (b < 0) return -1;
            got.mp[b] = qi; got.nmatches++;
            *new_occ = sc.obs[qi] > 0;
            return b;
        });
    CHECK(got == want);
    CHECK(rounds == ((sc.M > 0 && cam.N > 0) ? rounds_taken : 0) && rounds <= sc.M + 1);
    cov.scenes++; cov.exhausted += why.exhausted; cov.freed += why.freed;
}

static void two_cameras(const Scene& sc, bool device_built_right, Coverage& cov) {
    bool changed = false;
    const Result want = brute_two_cameras(sc, &changed);
    Result got = start(sc);
    Device dl(sc.cam[0], sc.qdesc), dr(sc.cam[1], sc.qdesc);
    std::vector<uint8_t> fl, fr;
    ClaimSide L = side_of(sc.cam[0], dl, got.occ[0], fl, false), R = side_of(sc.cam[1], dr, got.occ[1], fr, device_built_right);
    Why why;
    const int rc = replay_claims_two_cameras(L, R, sc.M, sc.obs.data(), sc.l2r.data(), sc.r2l.data(), got.mp.data(), kRatio,
        [&](int from) { why.note(L, dl, from, 2); if (L.N > 0) dl.round(L.occ, from); return 0; },
        [&](int from) { why.note(R, dr, from, 2); if (R.N > 0) dr.round(R.occ, from); return 0; }, &got.nmatches);
    CHECK(rc == 0);
    CHECK(got == want);
    CHECK(L.rounds >= 1 && R.rounds >= 1 && L.rounds <= sc.M + 1 && R.rounds <= sc.M + 1);
    cov.scenes++; cov.exhausted += why.exhausted; cov.freed += why.freed; cov.changed += changed;
}

static void report(const char* form, const Coverage& c, bool two) {
    const double e = 100.0 * c.exhausted / c.scenes, f = 100.0 * c.freed / c.scenes, ch = 100.0 * c.changed / c.scenes;
    std::printf("%-44s %d scenes: new round by an exhausted list %.0f %%, by a freed keypoint %.0f %%", form, c.scenes, e, f);
    if (two) std::printf(", side changed before its first query %.0f %%", ch);
    std::printf("\n");
    std::snprintf(g_where, sizeof g_where, "coverage of %s", form);
    CHECK(e >= 10.0 && f >= 10.0 && (!two || ch >= 10.0));
}

int main() {
    const int kScenes = 240;
    for (int device_built = 0; device_built < 2; device_built++) {
        Coverage ratio, threshold, rig;
        for (int s = 0; s < kScenes; s++) {
            std::snprintf(g_where, sizeof g_where, "scene %d, device-built queries %d", s, device_built);
            const Scene one = draw_scene(1000 + (uint64_t)s, s, false), two = draw_scene(900000 + (uint64_t)s, s, true);
            one_side(one, 2, device_built, s % 3 == 0, ratio);
            one_side(one, 1, device_built, s % 3 == 1, threshold);
            two_cameras(two, device_built, rig);
        }
        report(device_built ? "one side, ratio rule, device-built queries" : "one side, ratio rule", ratio, false);
        report(device_built ? "one side, threshold, device-built queries" : "one side, threshold", threshold, false);
        report(device_built ? "two cameras, right queries device-built" : "two cameras", rig, true);
    }
    std::printf("ok\n");
    return 0;
}
