// ms-slam_amd/host/Optimizer_device.h's LocalBundleAdjustment compiled against minimal stand-ins of KeyFrame / MapPoint / Map /
// Sophus::SE3f that carry the member names Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1040-1407) uses, linked to
// libmsorb.so through the C ABI.
//
//   dropin_localba in.bin out.bin
// in : K P E nlevels init_kf_id (int) | inv_level_sigma2[nlevels] (float) |
//      K x { q[4] t[3] fx fy cx cy mbf (float) local (int) } | P x { X Y Z (float) } | E x { kf point (int) x y u_right (float) octave (int) }
//      KeyFrame k has mnId 10 + k, point p mnId 500 + p; KeyFrame 0 is the one the routine is called for, the other `local` ones are
//      its covisible KeyFrames.  The program adds what the filters must drop: a bad covisible KeyFrame, a bad point and a point of
//      another map among KeyFrame 0's matches, and a point 902 whose only observation is at octave 11 (a local point without an edge).
// out: the gathered problem { K' P' E' (int) | K' x { mnId fixed (int) q[4] t[3] (float) } | P' x { mnId (int) } |
//      E' x { kf_index point_index (int) x y u_right inv_sigma2 (float) } } | ret num_fixedKF num_OptKF num_edges change_index (int) |
//      K x { q[4] t[3] (float) n_set_pose (int) } | P x { X Y Z (float) times_in_lba n_update (int) } | E x { still_observed (uint8) } |
//      second-camera run: ret n_set_pose_total change_index (int)
// Before that it runs GatherLocalBA on a graph of three KeyFrames and four points listed by hand in this file and compares the arrays
// with the ones listed beside it; a mismatch prints the array's name and exits with 4.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
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
struct KeyPoint { Point2f pt; float size, angle, response; int octave, class_id; };
struct Pinhole {};
struct Map {
    unsigned long init_id = 0;
    bool inertial = false;
    int change = 0;
    std::mutex mMutexMapUpdate;
    std::set<unsigned long> msOptKFs, msFixedKFs;
    unsigned long GetInitKFid() const { return init_id; }
    bool IsInertial() const { return inertial; }
    void IncreaseChangeIndex() { change++; }
};
constexpr unsigned long kNoMark = 1000000;
struct KeyFrame;
struct MapPoint;
typedef std::shared_ptr<KeyFrame> KFPtr;
typedef std::shared_ptr<MapPoint> MPPtr;
struct MapPoint {
    unsigned long mnId = 0, mnBALocalForKF = kNoMark;
    Map* map = nullptr;
    bool bad = false;
    Vec3f pos;
    std::map<KFPtr, std::tuple<int, int>> obs;
    int mnOptimizedTimesInLBA = 0, n_update = 0;
    bool isBad() const { return bad; }
    Map* GetMap() const { return map; }
    Vec3f GetWorldPos() const { return pos; }
    void SetWorldPos(const Vec3f& p) { pos = p; }
    void UpdateNormalAndDepth() { n_update++; }
    std::map<KFPtr, std::tuple<int, int>> GetObservations() const { return obs; }
    void EraseObservation(const KFPtr& k) { obs.erase(k); }
};
struct KeyFrame {
    unsigned long mnId = 0, mnBALocalForKF = kNoMark, mnBAFixedForKF = kNoMark;
    Map* map = nullptr;
    bool bad = false;
    std::vector<KFPtr> covisible;
    std::vector<MPPtr> mvpMapPoints;
    std::vector<KeyPoint> keys;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    Pinhole* mpCamera = nullptr;
    Pinhole* mpCamera2 = nullptr;
    SE3f Tcw;
    int n_set_pose = 0;
    bool isBad() const { return bad; }
    Map* GetMap() const { return map; }
    std::vector<KFPtr> GetVectorCovisibleKeyFrames() const { return covisible; }
    std::vector<MPPtr> GetMapPointMatches() const { return mvpMapPoints; }
    SE3f GetPose() const { return Tcw; }
    void SetPose(const SE3f& T) { Tcw = T; n_set_pose++; }
    float GetuRight(int i) const { return mvuRight[i]; }
    const KeyPoint& GetKeyUn(int i) const { return keys[i]; }
    void EraseMapPointMatch(const MPPtr& p) {
        for (auto& m : mvpMapPoints)
            if (m == p) m.reset();
    }
    int add_key(float x, float y, float ur, int octave, const MPPtr& p) {
        KeyPoint kp{};
        kp.pt.x = x; kp.pt.y = y; kp.octave = octave;
        keys.push_back(kp);
        mvuRight.push_back(ur);
        mvpMapPoints.push_back(p);
        return (int)keys.size() - 1;
    }
};

// KeyFrames in ONE block, so that the order of a map keyed by shared_ptr<KeyFrame> (the order of a point's edges) is the order here
struct Graph {
    std::vector<KeyFrame> store;
    std::vector<KFPtr> kf;
    std::vector<MPPtr> mp;
    Map map, other_map;
    Pinhole cam;
    explicit Graph(int K) : store(K) {
        for (int k = 0; k < K; k++) {
            kf.push_back(KFPtr(&store[k], [](KeyFrame*) {}));
            store[k].mnId = 10 + k;
            store[k].map = &map;
            store[k].mpCamera = &cam;
        }
    }
    ~Graph() {   // the KeyFrames and the points hold each other
        for (auto& p : mp) p->obs.clear();
        for (auto& k : store) { k.mvpMapPoints.clear(); k.covisible.clear(); }
    }
    MPPtr add_point(unsigned long id, float x, float y, float z) {
        MPPtr p = std::make_shared<MapPoint>();
        p->mnId = id; p->map = &map; p->pos = Vec3f(x, y, z);
        mp.push_back(p);
        return p;
    }
    void observe(int k, const MPPtr& p, float x, float y, float ur, int octave) {
        const int idx = kf[k]->add_key(x, y, ur, octave, p);
        p->obs[kf[k]] = std::make_tuple(idx, -1);
    }
};

template <class T>
bool same(const char* name, const std::vector<T>& got, const std::vector<T>& want) {
    if (got == want) return true;
    std::printf("hand-listed graph: %s differs (%zu entries, %zu expected)\n", name, got.size(), want.size());
    return false;
}

// three KeyFrames (10 = the current one, 11 covisible, 12 neither: a fixed camera), points 500..502 and a bad one
int hand_listed() {
    Graph G(3);
    G.map.init_id = 99;
    for (auto& k : G.store) { k.mvInvLevelSigma2 = {1.0f, 0.5f, 0.25f, 0.125f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.05f}; k.fx = k.fy = 700; k.cx = 600; k.cy = 180; k.mbf = 380; }
    G.kf[0]->covisible = {G.kf[1]};
    MPPtr p0 = G.add_point(500, 1, 2, 3), p1 = G.add_point(501, 4, 5, 6), p2 = G.add_point(502, 7, 8, 9), p3 = G.add_point(503, 0, 0, 1);
    p3->bad = true;
    G.observe(0, p0, 101, 102, 90, 0);
    G.observe(0, p1, 111, 112, -1, 1);
    G.observe(0, p3, 121, 122, -1, 0);
    G.observe(1, p0, 201, 202, -1, 2);
    G.observe(1, p2, 211, 212, 190, 3);
    G.observe(2, p1, 301, 302, 280, 0);
    G.observe(2, p2, 311, 312, -1, 11);   // octave > 10: no edge (:1220)
    auto B = ORB_SLAM3::msorb_host::GatherLocalBA(G.kf[0], &G.map);
    bool ok = B.num_fixedKF == 1 && B.lLocalKeyFrames.size() == 2 && B.lFixedCameras.size() == 1 && B.lLocalMapPoints.size() == 3 && !B.two_cameras;
    if (!ok) std::printf("hand-listed graph: the lists differ\n");
    std::vector<int> fixed, ids;
    for (const auto& k : B.kfs) fixed.push_back(k.fixed);
    for (const auto& k : B.kf_of_index) ids.push_back((int)k->mnId);
    ok &= same("KeyFrame ids", ids, {10, 11, 12});
    ok &= same("fixed", fixed, {0, 0, 1});
    ok &= same("edge_kf", B.edge_kf, {0, 1, 0, 2, 1});
    ok &= same("edge_point", B.edge_point, {0, 0, 1, 1, 2});
    ok &= same("xy", B.xy, {101, 102, 201, 202, 111, 112, 301, 302, 211, 212});
    ok &= same("u_right", B.u_right, {90, -1, -1, 280, 190});
    ok &= same("inv_sigma2", B.inv_sigma2, {1.0f, 0.25f, 0.5f, 1.0f, 0.125f});
    ok &= same("pos_w", B.pos_w, {1, 2, 3, 4, 5, 6, 7, 8, 9});
    ok &= B.kfs[2].fx == 700 && B.kfs[2].mbf == 380;
    // the marks go back where they were
    B.restore_marks();
    for (auto& k : G.store) ok &= k.mnBALocalForKF == kNoMark && k.mnBAFixedForKF == kNoMark;
    for (auto& p : G.mp) ok &= p->mnBALocalForKF == kNoMark;
    return ok ? 0 : 4;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    if (int rc = hand_listed()) return rc;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int dims[5];
    if (std::fread(dims, 4, 5, in) != 5) return 2;
    const int K = dims[0], P = dims[1], E = dims[2], nlevels = dims[3];
    std::vector<float> inv_level(nlevels);
    if (std::fread(inv_level.data(), 4, nlevels, in) != (size_t)nlevels) return 2;
    inv_level.resize(12, 0.01f);   // (so that the octave-11 keypoint below has an entry to be wrongly read from)
    auto build = [&](Graph& G, std::vector<std::pair<int, int>>& edges) -> bool {
        G.map.init_id = (unsigned long)dims[4];
        std::vector<int> local(K);
        for (int k = 0; k < K; k++) {
            float h[12];
            if (std::fread(h, 4, 12, in) != 12 || std::fread(&local[k], 4, 1, in) != 1) return false;
            KeyFrame& F = G.store[k];
            F.Tcw = SE3f(Quatf(h[3], h[0], h[1], h[2]), Vec3f(h[4], h[5], h[6]));
            F.fx = h[7]; F.fy = h[8]; F.cx = h[9]; F.cy = h[10]; F.mbf = h[11];
            F.mvInvLevelSigma2 = inv_level;
            if (k > 0 && local[k]) G.kf[0]->covisible.push_back(G.kf[k]);
        }
        for (int p = 0; p < P; p++) {
            float X[3];
            if (std::fread(X, 4, 3, in) != 3) return false;
            G.add_point(500 + p, X[0], X[1], X[2]);
        }
        for (int e = 0; e < E; e++) {
            int a[2], octave;
            float o[3];
            if (std::fread(a, 4, 2, in) != 2 || std::fread(o, 4, 3, in) != 3 || std::fread(&octave, 4, 1, in) != 1) return false;
            G.observe(a[0], G.mp[a[1]], o[0], o[1], o[2], octave);
            edges.push_back({a[0], a[1]});
        }
        // what the filters must drop
        KeyFrame& bad_kf = G.store[K];
        bad_kf.bad = true;
        bad_kf.mvInvLevelSigma2 = inv_level;
        G.kf[0]->covisible.push_back(G.kf[K]);
        MPPtr bad_point = G.add_point(900, 1, 1, 10), foreign = G.add_point(901, 1, 1, 12);
        bad_point->bad = true;
        foreign->map = &G.other_map;
        G.observe(0, bad_point, 50, 60, -1, 0);
        G.observe(0, foreign, 70, 80, -1, 0);
        G.observe(K, G.mp[0], 90, 100, -1, 0);      // the bad KeyFrame sees a local point
        G.observe(0, G.add_point(902, 2, 1, 14), 95, 105, -1, 11);   // octave 11: a local point (the last) whose only edge is dropped
        return true;
    };
    const long body = std::ftell(in);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    auto w_int = [&](int v) { std::fwrite(&v, 4, 1, out); };
    auto w_f = [&](float v) { std::fwrite(&v, 4, 1, out); };
    {
        Graph G(K + 1);
        std::vector<std::pair<int, int>> edges;
        if (!build(G, edges)) return 2;
        {   // the gathered problem, from a copy of the walk that leaves no marks
            auto B = ORB_SLAM3::msorb_host::GatherLocalBA(G.kf[0], &G.map);
            w_int((int)B.kfs.size()); w_int((int)B.lLocalMapPoints.size()); w_int((int)B.edge_kf.size());
            for (size_t k = 0; k < B.kfs.size(); k++) {
                w_int((int)B.kf_of_index[k]->mnId); w_int(B.kfs[k].fixed);
                for (int a = 0; a < 4; a++) w_f(B.kfs[k].q[a]);
                for (int a = 0; a < 3; a++) w_f(B.kfs[k].t[a]);
            }
            for (const auto& p : B.lLocalMapPoints) w_int((int)p->mnId);
            for (size_t e = 0; e < B.edge_kf.size(); e++) {
                w_int(B.edge_kf[e]); w_int(B.edge_point[e]);
                w_f(B.xy[2 * e]); w_f(B.xy[2 * e + 1]); w_f(B.u_right[e]); w_f(B.inv_sigma2[e]);
            }
            B.restore_marks();
        }
        bool stop = false;
        int num_fixed = -1, num_opt = -1, num_mps = -7, num_edges = -1;
        const bool ret = ORB_SLAM3::msorb_host::LocalBundleAdjustment(G.kf[0], &stop, &G.map, num_fixed, num_opt, num_mps, num_edges);
        if (num_mps != -7) return 5;   // the reference never writes it
        w_int(ret ? 1 : 0); w_int(num_fixed); w_int(num_opt); w_int(num_edges); w_int(G.map.change);
        for (int k = 0; k < K; k++) {
            const KeyFrame& F = G.store[k];
            w_f(F.Tcw.q.x()); w_f(F.Tcw.q.y()); w_f(F.Tcw.q.z()); w_f(F.Tcw.q.w());
            for (int a = 0; a < 3; a++) w_f(F.Tcw.t(a));
            w_int(F.n_set_pose);
        }
        for (int p = 0; p < P; p++) {
            for (int a = 0; a < 3; a++) w_f(G.mp[p]->pos(a));
            w_int(G.mp[p]->mnOptimizedTimesInLBA); w_int(G.mp[p]->n_update);
        }
        for (const auto& e : edges) {
            const uint8_t still = G.mp[e.second]->obs.count(G.kf[e.first]) ? 1 : 0;
            std::fwrite(&still, 1, 1, out);
        }
    }
    {   // a KeyFrame of the problem has a second camera: false, nothing touched, the marks as they were
        std::fseek(in, body, SEEK_SET);
        Graph G(K + 1);
        std::vector<std::pair<int, int>> edges;
        if (!build(G, edges)) return 2;
        G.store[K - 1].mpCamera2 = &G.cam;
        bool stop = false;
        int a = -1, b = -1, c = -1, d = -1;
        const bool ret = ORB_SLAM3::msorb_host::LocalBundleAdjustment(G.kf[0], &stop, &G.map, a, b, c, d);
        int n_set = 0, marks = 0;
        for (auto& k : G.store) { n_set += k.n_set_pose; marks += k.mnBALocalForKF != kNoMark || k.mnBAFixedForKF != kNoMark; }
        for (auto& p : G.mp) { n_set += p->mnOptimizedTimesInLBA; marks += p->mnBALocalForKF != kNoMark; }
        w_int(ret ? 1 : 0); w_int(n_set + marks); w_int(G.map.change);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
