// ms-slam_amd/host/Optimizer_device.h's welding LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag) compiled against
// minimal stand-ins of KeyFrame / MapPoint / Map / Sophus::SE3f that carry the member names the second
// Optimizer::LocalBundleAdjustment (src/Optimizer.cc:3494-3915) uses, linked to libmsorb.so through the C ABI.  The program makes its
// own small map (two fixed KeyFrames 10, 11, three adjustable ones 12..14, sixty points seen by three or four of them, mono and
// stereo mixed, every seventh observation of the adjustable KeyFrames with a gross error) and adds what the filters must drop: a
// bad adjustable KeyFrame 15 with observations, an adjustable KeyFrame 16 of another map, a KeyFrame 17 that is in neither list, a
// bad point, a point of another map, an observation at octave 11, and an observation whose slot in the KeyFrame is empty.  Every
// check compares what the routine did to the map with what msorb_welding_ba returns for the arrays listed beside it.  Prints "ok"
// and exits with 0, or names the check that failed and exits with 1.
//
//   dropin_welding_ba            all checks (needs the device)
//   dropin_welding_ba --gather   built with -DWELDING_BA_GATHER_ONLY, without the library: the gathering walk against the listed
//                                arrays and the stop-flag mirror alone, which is what runs under the sanitizers
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <thread>
#include <tuple>
#include <vector>

#include "Optimizer_device.h"

namespace {

struct Vec3f {
    float v[3];
    Vec3f() : v{0, 0, 0} {}
    Vec3f(float x, float y, float z) : v{x, y, z} {}
    float operator()(int i) const { return v[i]; }
};
struct Quatf {
    float w_, x_, y_, z_;
    Quatf() : w_(1), x_(0), y_(0), z_(0) {}
    Quatf(float w, float x, float y, float z) : w_(w), x_(x), y_(y), z_(z) {}   // Eigen's argument order
    float x() const { return x_; }
    float y() const { return y_; }
    float z() const { return z_; }
    float w() const { return w_; }
};
struct SE3f {   // Sophus::SE3<float> as far as the routine uses it (no normalisation here: what SetPose receives is what is stored)
    Quatf q;
    Vec3f t;
    SE3f() {}
    SE3f(const Quatf& q_, const Vec3f& t_) : q(q_), t(t_) {}
    const Quatf& unit_quaternion() const { return q; }
    const Vec3f& translation() const { return t; }
};
struct Point2f { float x, y; };
struct KeyPoint { Point2f pt; int octave; };
struct Camera {
    enum { CAM_PINHOLE = 0, CAM_FISHEYE = 1 };
    int type = CAM_PINHOLE;
    int GetType() const { return type; }
};
struct KeyFrame;
struct MapPoint;
typedef std::shared_ptr<KeyFrame> KFPtr;
typedef std::shared_ptr<MapPoint> MPPtr;
struct Map { std::mutex mMutexMapUpdate; };
constexpr unsigned long kNoMark = 1000000;
struct MapPoint {
    unsigned long mnId = 0, mnBALocalForMerge = kNoMark;
    Map* map = nullptr;
    bool bad = false;
    Vec3f pos;
    std::map<KFPtr, std::tuple<int, int>> obs;
    int n_set = 0, n_update = 0, n_erase = 0;
    bool isBad() const { return bad; }
    Map* GetMap() const { return map; }
    Vec3f GetWorldPos() const { return pos; }
    void SetWorldPos(const Vec3f& p) { pos = p; n_set++; }
    void UpdateNormalAndDepth() { n_update++; }
    std::map<KFPtr, std::tuple<int, int>> GetObservations() const { return obs; }
    void EraseObservation(const KFPtr& k) { obs.erase(k); n_erase++; }
};
struct KeyFrame {
    unsigned long mnId = 0, mnBALocalForMerge = kNoMark;
    Map* map = nullptr;
    bool bad = false;
    std::vector<KeyPoint> keys;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<MPPtr> mvpMapPoints;
    float fx = 700, fy = 700, cx = 600, cy = 180, mbf = 380;
    Camera* mpCamera = nullptr;
    Camera* mpCamera2 = nullptr;
    SE3f Tcw;
    int n_set_pose = 0, n_erase = 0;
    bool isBad() const { return bad; }
    Map* GetMap() const { return map; }
    SE3f GetPose() const { return Tcw; }
    void SetPose(const SE3f& T) { Tcw = T; n_set_pose++; }
    float GetuRight(int i) const { return mvuRight[i]; }
    const KeyPoint& GetKeyUn(int i) const { return keys[i]; }
    MPPtr GetMapPoint(int i) const { return mvpMapPoints[i]; }
    std::set<MPPtr> GetMapPoints() const {
        std::set<MPPtr> s;
        for (const MPPtr& p : mvpMapPoints)
            if (p) s.insert(p);
        return s;
    }
    void EraseMapPointMatch(const MPPtr& p) {
        for (auto& m : mvpMapPoints)
            if (m == p) { m.reset(); n_erase++; }
    }
};

constexpr int kFixed = 2, kAdjust = 3, kGood = kFixed + kAdjust, kAll = 8, kPoints = 60, kAllPoints = kPoints + 4;

// KeyFrames and points in ONE block each, so that the order of a set or a map keyed by a shared_ptr is the order here
struct World {
    std::vector<KeyFrame> store;    // 0, 1 fixed; 2..4 adjustable; 5 adjustable and bad; 6 adjustable, of another map; 7 in no list
    std::vector<MapPoint> pstore;   // 0..59 good; 60 bad; 61 of another map; 62 seen at octave 11 only; 63 seen by 12 through an empty slot, and by 13
    std::vector<KFPtr> kf;
    std::vector<MPPtr> mp;
    Map map, other;
    Camera cam, fisheye;
    std::vector<KFPtr> adjust, fixed;
    // the arrays the routine has to gather
    std::vector<msorb_ba_keyframe> kfs;
    std::vector<float> pos_w, xy, ur, inv;
    std::vector<int> ek, ep, point_of;          // point_of [kAllPoints]: the vertex of a point, -1 none
    std::vector<std::pair<int, int>> edge_kp;   // (KeyFrame, point) per listed edge

    static unsigned rnd(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
    static float uni(unsigned& s) { return (float)(rnd(s) % 20001) / 10000.0f - 1.0f; }

    void observe(int k, int p, float x, float y, float u_right, int octave, bool empty_slot = false) {
        KeyPoint kp{{x, y}, octave};
        store[k].keys.push_back(kp);
        store[k].mvuRight.push_back(u_right);
        store[k].mvpMapPoints.push_back(empty_slot ? MPPtr() : mp[p]);
        mp[p]->obs[kf[k]] = std::make_tuple((int)store[k].keys.size() - 1, -1);
    }
    World() : store(kAll), pstore(kAllPoints) {
        fisheye.type = Camera::CAM_FISHEYE;
        unsigned seed = 4321;
        for (int k = 0; k < kAll; k++) {
            kf.push_back(KFPtr(&store[k], [](KeyFrame*) {}));
            KeyFrame& f = store[k];
            f.mnId = 10 + k;
            f.map = k == 6 ? &other : &map;
            f.mpCamera = &cam;
            f.mvInvLevelSigma2 = {1.0f, 0.69444f, 0.48225f, 0.33490f, 0.2f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.05f};
            const float ax = 0.02f * uni(seed), ay = 0.03f * uni(seed), az = 0.02f * uni(seed);   // a small rotation, not normalised to the last bit
            const float w = std::sqrt(1 - ax * ax - ay * ay - az * az);
            f.Tcw = SE3f(Quatf(w, ax, ay, az), Vec3f(0.8f * uni(seed), 0.2f * uni(seed), 0.5f * uni(seed)));
        }
        store[5].bad = true;
        for (int p = 0; p < kAllPoints; p++) {
            mp.push_back(MPPtr(&pstore[p], [](MapPoint*) {}));
            pstore[p].mnId = 500 + p;
            pstore[p].map = p == kPoints + 1 ? &other : &map;
            const float z = 8 + 12 * (uni(seed) + 1);
            pstore[p].pos = Vec3f(6 * uni(seed), 2 * uni(seed), z);
        }
        pstore[kPoints].bad = true;
        for (int k = 0; k < kGood; k++) {
            msorb_ba_keyframe r;
            const KeyFrame& f = store[k];
            r.q[0] = f.Tcw.q.x(); r.q[1] = f.Tcw.q.y(); r.q[2] = f.Tcw.q.z(); r.q[3] = f.Tcw.q.w();
            for (int a = 0; a < 3; a++) r.t[a] = f.Tcw.t(a);
            r.fx = f.fx; r.fy = f.fy; r.cx = f.cx; r.cy = f.cy; r.mbf = f.mbf;
            r.fixed = k < kFixed;
            kfs.push_back(r);
        }
        struct Seen { int k; float u, v, u_r; int octave; bool empty_slot; };
        std::vector<std::vector<Seen>> seen((size_t)kAllPoints);
        int count = 0;
        for (int p = 0; p < kAllPoints; p++)
            for (int k = 0; k < kAll; k++) {
                bool sees = (p + k) % 5 != 0 || k >= kGood;     // four of the five good KeyFrames, and the three others
                if (p == kPoints + 2) sees = k == 2;
                if (p == kPoints + 3) sees = k == 2 || k == 3;
                if (!sees) continue;
                // the pinhole image under the KeyFrame's pose (rotation to first order is enough for a test scene), plus an error
                const KeyFrame& f = store[k];
                const float X = pstore[p].pos(0), Y = pstore[p].pos(1), Z = pstore[p].pos(2);
                const float xc = X + 2 * (f.Tcw.q.y() * Z - f.Tcw.q.z() * Y) + f.Tcw.t(0), yc = Y + 2 * (f.Tcw.q.z() * X - f.Tcw.q.x() * Z) + f.Tcw.t(1),
                            zc = Z + 2 * (f.Tcw.q.x() * Y - f.Tcw.q.y() * X) + f.Tcw.t(2);
                float u = f.fx * xc / zc + f.cx + 2 * uni(seed), v = f.fy * yc / zc + f.cy + 2 * uni(seed);
                const bool stereo = (p + 2 * k) % 3 == 0;
                const float u_r = stereo ? u - f.mbf / zc + uni(seed) : -1.0f;
                if (k >= kFixed && k < kGood && p < kPoints && ++count % 7 == 0) { u += 90; v -= 70; }   // a gross error
                const int octave = p == kPoints + 2 ? 11 : (p + k) % 4;
                const bool empty_slot = p == kPoints + 3 && k == 2;
                observe(k, p, u, v, u_r, octave, empty_slot);
                seen[p].push_back(Seen{k, u, v, u_r, octave, empty_slot});
            }
        // what the walk of :3515-3707 makes of it: the points in the order in which the KeyFrames list them (fixed first), a
        // point's edges in the order of its observations (the KeyFrames ascending)
        point_of.assign((size_t)kAllPoints, -1);
        int n_points = 0;
        std::vector<int> order;
        for (int k = 0; k < kGood; k++)
            for (int p = 0; p < kAllPoints; p++) {
                if (point_of[p] >= 0 || p == kPoints || p == kPoints + 1) continue;                      // listed, bad, of another map
                bool sees = false;
                for (const Seen& s : seen[p]) sees |= s.k == k && !s.empty_slot;
                if (!sees) continue;
                point_of[p] = n_points++;
                order.push_back(p);
            }
        for (int p : order) {
            pos_w.push_back(pstore[p].pos(0)); pos_w.push_back(pstore[p].pos(1)); pos_w.push_back(pstore[p].pos(2));
            for (const Seen& s : seen[p]) {
                if (s.k >= kGood || s.octave > 10 || s.empty_slot) continue;   // KeyFrames 15 (bad), 16 (another map), 17 (no list); octave 11; :3634
                ek.push_back(s.k);
                ep.push_back(point_of[p]);
                xy.push_back(s.u); xy.push_back(s.v);
                ur.push_back(s.u_r);
                inv.push_back(store[s.k].mvInvLevelSigma2[s.octave]);
                edge_kp.push_back({s.k, p});
            }
        }
        for (int k = 0; k < kFixed; k++) fixed.push_back(kf[k]);
        for (int k = kFixed; k < 7; k++) adjust.push_back(kf[k]);
    }
    ~World() {   // the KeyFrames and the points hold each other
        for (auto& p : pstore) p.obs.clear();
        for (auto& k : store) k.mvpMapPoints.clear();
    }
    bool marks_are(unsigned long id) const {   // the walk's marks: the five KeyFrames and every listed point
        for (int k = 0; k < kAll; k++)
            if (store[k].mnBALocalForMerge != (k < kGood ? id : kNoMark)) return false;
        for (int p = 0; p < kAllPoints; p++)
            if (pstore[p].mnBALocalForMerge != (point_of[p] >= 0 ? id : kNoMark)) return false;
        return true;
    }
    int setters() const {
        int n = 0;
        for (const auto& k : store) n += k.n_set_pose + k.n_erase;
        for (const auto& p : pstore) n += p.n_set + p.n_update + p.n_erase;
        return n;
    }
};

#define CHECK(cond) do { if (!(cond)) { std::printf("%s: failed: %s (line %d)\n", what, #cond, __LINE__); return false; } } while (0)

bool gathered(const char* what) {
    World W;
    const auto B = ORB_SLAM3::msorb_host::GatherWeldingBA(W.kf[2], W.adjust, W.fixed);
    CHECK(B.pinhole && B.n_free == kAdjust && B.kfs.size() == W.kfs.size());
    CHECK(std::memcmp(B.kfs.data(), W.kfs.data(), W.kfs.size() * sizeof(msorb_ba_keyframe)) == 0);
    CHECK(B.pos_w == W.pos_w && B.edge_kf == W.ek && B.edge_point == W.ep && B.xy == W.xy && B.u_right == W.ur && B.inv_sigma2 == W.inv);
    CHECK(B.edge_objects.size() == W.ek.size() && W.ek.size() > 150 && W.pos_w.size() == 3 * (size_t)(kPoints + 2));
    for (size_t e = 0; e < W.ek.size(); e++) CHECK(B.edge_objects[e].first == W.kf[W.edge_kp[e].first] && B.edge_objects[e].second == W.mp[W.edge_kp[e].second]);
    CHECK(W.point_of[kPoints + 2] >= 0 && W.point_of[kPoints + 3] >= 0);   // octave 11 alone: a vertex without an edge; the empty slot: one edge, KeyFrame 13's
    CHECK(std::count(W.ep.begin(), W.ep.end(), W.point_of[kPoints + 2]) == 0 && std::count(W.ep.begin(), W.ep.end(), W.point_of[kPoints + 3]) == 1);
    CHECK(W.marks_are(12) && W.setters() == 0);
    auto C = B;
    C.restore_marks();
    CHECK(W.marks_are(kNoMark));
    return true;
}

// the bool another thread sets reaches the int the C ABI reads; a NULL flag is NULL; a flag that is already set is seen at once
bool mirrored(const char* what) {
    using ORB_SLAM3::msorb_host::StopFlagMirror;
    {
        StopFlagMirror none(nullptr);
        CHECK(none.get() == nullptr);
    }
    {
        bool flag = true;
        StopFlagMirror set(&flag);
        CHECK(set.get() && *set.get() == 1);
    }
    {
        bool flag = false;
        StopFlagMirror live(&flag);
        CHECK(live.get() && *live.get() == 0);
        std::thread setter([&] { *static_cast<volatile bool*>(&flag) = true; });
        setter.join();
        for (int i = 0; i < 2000 && !*live.get(); i++) std::this_thread::sleep_for(std::chrono::milliseconds(1));
        CHECK(*live.get() == 1);
    }
    {
        bool flag = false;   // one that stays clear: the watcher ends with the object
        StopFlagMirror clear(&flag);
        CHECK(*clear.get() == 0);
    }
    return true;
}

#ifndef WELDING_BA_GATHER_ONLY
bool same_pose(const SE3f& T, const float* o) {
    const float got[7] = {T.q.x(), T.q.y(), T.q.z(), T.q.w(), T.t(0), T.t(1), T.t(2)};
    return std::memcmp(got, o, sizeof got) == 0;
}
bool same_pos(const Vec3f& p, const float* o) { return std::memcmp(p.v, o, 12) == 0; }

struct Expected {
    std::vector<float> kf_out, pos_out;
    std::vector<uint8_t> level1, outlier;
    msorb_welding_ba_result r;
    Expected(const World& W, const int* stop) {
        const int K = (int)W.kfs.size(), P = (int)W.pos_w.size() / 3, E = (int)W.ek.size();
        kf_out.assign(7 * (size_t)K, 0);
        pos_out.assign(3 * (size_t)P, 0);
        level1.assign((size_t)E, 0);
        outlier.assign((size_t)E, 0);
        if (msorb_welding_ba(0, K, W.kfs.data(), P, W.pos_w.data(), E, W.ek.data(), W.ep.data(), W.xy.data(), W.ur.data(), W.inv.data(), stop,
                             kf_out.data(), nullptr, pos_out.data(), nullptr, level1.data(), outlier.data(), &r, nullptr) != MSORB_OK) {
            std::printf("msorb_welding_ba: %s\n", msorb_last_error());
            std::exit(2);
        }
    }
};

bool applied(const char* what, bool* stop_flag) {
    World W, fresh;
    const Expected X(W, nullptr);
    CHECK(X.r.status == 0 && X.r.round[0].iterations == 5 && X.r.round[1].iterations > 0 && X.r.n_outliers > 0 && X.r.n_level1 > 0);
    CHECK(ORB_SLAM3::msorb_host::LocalBundleAdjustment(W.kf[2], W.adjust, W.fixed, stop_flag));
    CHECK(W.marks_are(12));
    for (int k = 0; k < kAll; k++) {
        const bool adj = k >= kFixed && k < kGood;
        CHECK(W.store[k].n_set_pose == (adj ? 1 : 0));
        if (adj) CHECK(same_pose(W.store[k].Tcw, &X.kf_out[7 * k]) && !same_pose(W.store[k].Tcw, &fresh.kfs[k].q[0]));
        else CHECK(std::memcmp(&W.store[k].Tcw, &fresh.store[k].Tcw, sizeof(SE3f)) == 0);
    }
    for (int p = 0; p < kAllPoints; p++) {
        const int v = W.point_of[p];
        CHECK(W.pstore[p].n_set == (v >= 0) && W.pstore[p].n_update == (v >= 0));
        if (v >= 0) CHECK(same_pos(W.pstore[p].pos, &X.pos_out[3 * v]));
        else CHECK(same_pos(W.pstore[p].pos, fresh.pstore[p].pos.v));
    }
    CHECK(same_pos(W.pstore[kPoints + 2].pos, fresh.pstore[kPoints + 2].pos.v));   // the vertex without an edge: set to where it was
    // the erased observations are the flagged edges, and no other
    int erased = 0;
    for (size_t e = 0; e < W.ek.size(); e++) {
        const int k = W.edge_kp[e].first, p = W.edge_kp[e].second;
        const bool still = W.pstore[p].obs.count(W.kf[k]) != 0;
        CHECK(still == !X.outlier[e]);
        bool slot = false;
        for (const MPPtr& m : W.store[k].mvpMapPoints) slot |= m == W.mp[p];
        CHECK(slot == still);
        erased += !still;
    }
    CHECK(erased == X.r.n_outliers);
    int calls = 0;
    for (const auto& k : W.store) calls += k.n_erase;
    for (const auto& p : W.pstore) calls -= p.n_erase;
    CHECK(calls == 0);
    for (int k = kGood; k < kAll; k++) CHECK(W.store[k].n_erase == 0);
    return true;
}

bool stopped(const char* what) {
    World W, fresh;
    bool stop = true;
    const int one = 1;
    const Expected X(W, &one);
    CHECK(X.r.status == 2);
    CHECK(ORB_SLAM3::msorb_host::LocalBundleAdjustment(W.kf[2], W.adjust, W.fixed, &stop));
    CHECK(W.marks_are(12) && W.setters() == 0);
    for (int k = 0; k < kAll; k++) CHECK(std::memcmp(&W.store[k].Tcw, &fresh.store[k].Tcw, sizeof(SE3f)) == 0);
    return true;
}

// the flag raised between the rounds through the library's poll hook: status 3, round 1's counts, no level, the flags of the one
// classification (the levels of the undisturbed call), and the estimates of round 1: the engine's own optimize(5) with kernels
void raise_between(void* user, int, int where, int, int) {
    if (where == MSORB_WELDING_POLL_BETWEEN) *static_cast<volatile int*>(user) = 1;
}
bool between(const char* what) {
    World W;
    const Expected X(W, nullptr);
    int flag = 0;
    msorb_debug_welding_ba_poll_hook(raise_between, &flag);
    const Expected S(W, &flag);
    msorb_debug_welding_ba_poll_hook(nullptr, nullptr);
    CHECK(flag == 1 && S.r.status == 3 && S.r.n_level1 == 0 && S.r.active_keyframes == 0 && S.r.active_points == 0);
    CHECK(S.r.round[0].iterations == X.r.round[0].iterations && S.r.round[0].trials == X.r.round[0].trials);
    CHECK(S.r.round[0].chi2_final == X.r.round[0].chi2_final && S.r.round[0].lambda_final == X.r.round[0].lambda_final);
    CHECK(S.r.round[1].iterations == 0 && S.r.round[1].trials == 0 && S.r.round[1].chi2_initial == 0);
    int set = 0;
    for (size_t e = 0; e < S.outlier.size(); e++) {
        CHECK(S.level1[e] == 0 && S.outlier[e] == X.level1[e]);
        set += S.outlier[e];
    }
    CHECK(set == X.r.n_level1 && set == S.r.n_outliers && set > 0);
    const int K = (int)W.kfs.size(), P = (int)W.pos_w.size() / 3, E = (int)W.ek.size();
    std::vector<float> kf_out(7 * (size_t)K), pos_out(3 * (size_t)P);
    std::vector<uint8_t> inc((size_t)P);
    msorb_ba_result one;
    CHECK(msorb_bundle_adjustment(0, K, W.kfs.data(), P, W.pos_w.data(), E, W.ek.data(), W.ep.data(), W.xy.data(), W.ur.data(), W.inv.data(), 5, 1,
                                  nullptr, kf_out.data(), nullptr, pos_out.data(), nullptr, inc.data(), &one, nullptr) == MSORB_OK);
    CHECK(one.iterations == S.r.round[0].iterations && one.chi2_final == S.r.round[0].chi2_final);
    CHECK(kf_out == S.kf_out && S.kf_out != X.kf_out);
    for (int p = 0; p < P; p++)
        if (inc[p]) CHECK(std::memcmp(&pos_out[3 * p], &S.pos_out[3 * p], 12) == 0);
    // and the hook is gone: the next call is the undisturbed one
    flag = 0;
    const Expected Y(W, &flag);
    CHECK(flag == 0 && Y.r.status == 0 && Y.kf_out == X.kf_out && Y.outlier == X.outlier);
    return true;
}

bool refused(const char* what) {
    {   // a camera that is not a pinhole
        World W;
        W.store[3].mpCamera = &W.fisheye;
        CHECK(!ORB_SLAM3::msorb_host::LocalBundleAdjustment(W.kf[2], W.adjust, W.fixed, nullptr));
        CHECK(W.marks_are(kNoMark) && W.setters() == 0);
    }
    {   // more adjustable KeyFrames than the capacity
        World W;
        const int extra = msorb_welding_ba_capacity() + 1;
        std::vector<KeyFrame> more((size_t)extra);
        std::vector<KFPtr> adjust = W.adjust;
        for (int k = 0; k < extra; k++) {
            more[k].mnId = 100 + k;
            more[k].map = &W.map;
            more[k].mpCamera = &W.cam;
            adjust.push_back(KFPtr(&more[k], [](KeyFrame*) {}));
        }
        CHECK(!ORB_SLAM3::msorb_host::LocalBundleAdjustment(W.kf[2], adjust, W.fixed, nullptr));
        for (const KeyFrame& k : more) CHECK(k.n_set_pose == 0 && k.mnBALocalForMerge == kNoMark);
        CHECK(W.marks_are(kNoMark) && W.setters() == 0);
    }
    return true;
}
#endif

}  // namespace

int main(int argc, char** argv) {
    bool ok = gathered("the gathering walk") && mirrored("the stop-flag mirror");
#ifndef WELDING_BA_GATHER_ONLY
    if (argc < 2 || std::strcmp(argv[1], "--gather") != 0) {
        bool go = false;
        ok = ok && applied("LocalBundleAdjustment (welding)", nullptr) && applied("a stop flag that stays clear", &go) &&
             stopped("a stop flag that is set") && between("a stop flag raised between the rounds") && refused("not handled");
    }
#else
    (void)argc; (void)argv;
#endif
    if (ok) std::printf("ok\n");
    return ok ? 0 : 1;
}
