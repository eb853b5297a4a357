// ms-slam_amd/host/Optimizer_device.h's MergeInertialBA compiled against minimal stand-ins of KeyFrame / MapPoint / Map /
// IMU::Preintegrated / IMU::Bias / Sophus::SE3f / g2o::Sim3 that carry the member names Optimizer::MergeInertialBA
// (src/Optimizer.cc:3918-4420) uses, linked to libmsorb.so through the C ABI.
//
//   dropin_merge_inertial_ba in.bin out.bin
//   dropin_merge_inertial_ba --hand           the hand-listed graphs, the refusals and the flag found set, alone (no device)
// in : tests/merge_inertial_ba_cases.py's write_dropin_scene: int32 K, NI, P, E, the index of pCurrKF, of pMergeKF, then
//      msorb_iba_keyframe [K] (ascending mnId), msorb_iba_inertial_edge [NI] (pre.kf_prev / kf_cur name the KeyFrames), the 15 x 15
//      float covariance of every edge, pos_w [3 P], edge_kf [E], edge_point [E], xy [2 E], u_right [E], octave [E] (int32),
//      mvInvLevelSigma2 [8].  KeyFrame k has mnId 10 + k, point p mnId 500 + p.
// out: the gathered problem in merge_inertial_ba_cases' write_scenes layout, the gathered points' scene indices [P'] (int32), then
//      ret, change_index, n_SetNewBias on preintegrations (int32), per KeyFrame { n_set_pose n_set_velocity n_set_bias has_corr
//      (int32) Rcw[9] tcw[3] v[3] bias[6] as the setters left them (float), corrPoses' rotation[9] translation[3] scale (double) },
//      per point { n_set_pos n_update (int32) pos[3] }, per edge of the input whether its observation is still there (uint8).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "Optimizer_device.h"

namespace {

struct Vec3f {
    float v[3];
    Vec3f() : v{0, 0, 0} {}
    Vec3f(float x, float y, float z) : v{x, y, z} {}
    float operator()(int i) const { return v[i]; }
    float& operator()(int i) { return v[i]; }
};
struct Mat3f {
    float m[9];
    Mat3f() : m{1, 0, 0, 0, 1, 0, 0, 0, 1} {}
    float operator()(int r, int c) const { return m[3 * r + c]; }
    float& operator()(int r, int c) { return m[3 * r + c]; }
};
struct Mat15f {
    float m[225] = {0};
    float operator()(int r, int c) const { return m[15 * r + c]; }
};
struct Rotd { double m[9]; };      // what the stand-in keeps of a unit quaternion: the rotation it stands for, widened
struct Vec3d { double v[3]; };
struct SE3d {
    Rotd R;
    Vec3d t;
    Rotd unit_quaternion() const { return R; }
    Vec3d translation() const { return t; }
};
struct SE3f {   // Sophus::SE3<float> as far as the routine uses it
    Mat3f R;
    Vec3f t;
    SE3f() {}
    SE3f(const Mat3f& R_, const Vec3f& t_) : R(R_), t(t_) {}
    Mat3f rotationMatrix() const { return R; }
    Vec3f translation() const { return t; }
    template <class T>
    SE3d cast() const {
        SE3d o;
        for (int i = 0; i < 9; i++) o.R.m[i] = (T)R.m[i];
        for (int i = 0; i < 3; i++) o.t.v[i] = (T)t.v[i];
        return o;
    }
};
struct Sim3 {   // g2o::Sim3(q, t, s)
    Rotd r{};
    Vec3d t{};
    double s = 0;
    Sim3() {}
    Sim3(const Rotd& r_, const Vec3d& t_, double s_) : r(r_), t(t_), s(s_) {}
};
struct Bias {
    float bax = 0, bay = 0, baz = 0, bwx = 0, bwy = 0, bwz = 0;
    Bias() {}
    Bias(float ax, float ay, float az, float wx, float wy, float wz) : bax(ax), bay(ay), baz(az), bwx(wx), bwy(wy), bwz(wz) {}
};
struct Preintegrated {
    Mat3f dR, JRg, JVg, JVa, JPg, JPa;
    Vec3f dV, dP;
    Mat15f C;
    Bias b, bu;
    float dT = 0;
    int n_set_new_bias = 0;
    void SetNewBias(const Bias& nb) { bu = nb; n_set_new_bias++; }
};
struct Calib { SE3f mTcb, mTbc; };
struct Point2f { float x, y; };
struct KeyPoint { Point2f pt; float size, angle, response; int octave, class_id; };
struct Pinhole {};
struct KeyFrame;
struct MapPoint;
typedef std::shared_ptr<KeyFrame> KFPtr;
typedef std::shared_ptr<MapPoint> MPPtr;
struct Map {
    int change = 0;
    std::mutex mMutexMapUpdate;
    void IncreaseChangeIndex() { change++; }
};
struct MapPoint {
    unsigned long mnId = 0, mnBALocalForKF = 0;
    bool bad = false;
    Vec3f pos;
    std::map<KFPtr, std::tuple<int, int>> obs;
    int n_set_pos = 0, n_update = 0;
    bool isBad() const { return bad; }
    Vec3f GetWorldPos() const { return pos; }
    void SetWorldPos(const Vec3f& p) { pos = p; n_set_pos++; }
    void UpdateNormalAndDepth() { n_update++; }
    std::map<KFPtr, std::tuple<int, int>> GetObservations() const { return obs; }
    void EraseObservation(const KFPtr& k) { obs.erase(k); }
};
struct KeyFrame {
    unsigned long mnId = 0, mnBALocalForKF = 0, mnBAFixedForKF = 0;
    bool bad = false, bImu = true;
    KFPtr mPrevKF, mNextKF;
    Preintegrated* mpImuPreintegrated = nullptr;
    std::vector<MPPtr> mvpMapPoints;
    std::vector<KeyPoint> keys;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    Pinhole* mpCamera = nullptr;
    Pinhole* mpCamera2 = nullptr;
    Calib mImuCalib;
    SE3f Tcw;
    Mat3f Rwb;
    Vec3f twb, vel;
    Bias bias;
    int n_set_pose = 0, n_set_velocity = 0, n_set_bias = 0;
    bool isBad() const { return bad; }
    std::vector<MPPtr> GetMapPointMatches() const { return mvpMapPoints; }
    SE3f GetPose() const { return Tcw; }
    Mat3f GetImuRotation() const { return Rwb; }
    Vec3f GetImuPosition() const { return twb; }
    Vec3f GetVelocity() const { return vel; }
    Vec3f GetGyroBias() const { return Vec3f(bias.bwx, bias.bwy, bias.bwz); }
    Vec3f GetAccBias() const { return Vec3f(bias.bax, bias.bay, bias.baz); }
    Bias GetImuBias() const { return bias; }
    void SetPose(const SE3f& T) { Tcw = T; n_set_pose++; }
    void SetVelocity(const Vec3f& v) { vel = v; n_set_velocity++; }
    void SetNewBias(const Bias& b) { bias = b; n_set_bias++; }
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
typedef std::map<KFPtr, Sim3> KeyFrameAndPose;

// KeyFrames and points in ONE block each, so that the order of a map keyed by a shared_ptr is the order here
struct Graph {
    std::vector<KeyFrame> store;
    std::vector<MapPoint> pstore;
    std::vector<Preintegrated> pre;
    std::vector<KFPtr> kf;
    std::vector<MPPtr> mp;
    Map map;
    Pinhole cam;
    Graph(int K, int P) : store(K), pstore(P), pre(K) {
        for (int k = 0; k < K; k++) {
            kf.push_back(KFPtr(&store[k], [](KeyFrame*) {}));
            store[k].mnId = 10 + k;
            store[k].mpCamera = &cam;
            store[k].fx = store[k].fy = 700; store[k].cx = 600; store[k].cy = 180; store[k].mbf = 380;
            store[k].mvInvLevelSigma2 = {1.0f, 0.5f, 0.25f, 0.125f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.05f};
            for (int q = 0; q < 15; q++) pre[k].C.m[16 * q] = 1e-4f * (1 + q);   // an invertible covariance
        }
        for (int p = 0; p < P; p++) {
            mp.push_back(MPPtr(&pstore[p], [](MapPoint*) {}));
            pstore[p].mnId = 500 + p;
            pstore[p].pos = Vec3f(1.f + p, 2.f, 3.f);
        }
    }
    ~Graph() {   // the KeyFrames and the points hold each other
        for (auto& p : pstore) p.obs.clear();
        for (auto& k : store) { k.mvpMapPoints.clear(); k.mPrevKF.reset(); k.mNextKF.reset(); }
    }
    void link(int k, int prev) { store[k].mPrevKF = kf[prev]; store[k].mpImuPreintegrated = &pre[k]; }
    void observe(int k, int p, float x, float y, float ur, int octave) {
        const int idx = kf[k]->add_key(x, y, ur, octave, mp[p]);
        mp[p]->obs[kf[k]] = std::make_tuple(idx, -1);
    }
    int touched(bool marks) const {   // setters, SetNewBias on a preintegration, the change index, and the marks of the walk
        int n = map.change;
        for (const auto& k : store) n += k.n_set_pose + k.n_set_velocity + k.n_set_bias + (marks ? (k.mnBALocalForKF != 0) + (k.mnBAFixedForKF != 0) : 0);
        for (const auto& q : pre) n += q.n_set_new_bias;
        for (const auto& p : pstore) n += p.n_set_pos + p.n_update + (marks ? (p.mnBALocalForKF != 0) : 0);
        return n;
    }
};

template <class T>
bool same(const char* name, const std::vector<T>& got, const std::vector<T>& want) {
    if (got == want) return true;
    std::printf("hand-listed graph: %s differs (%zu entries, %zu expected):", name, got.size(), want.size());
    for (const T& v : got) std::printf(" %g", (double)v);
    std::printf("\n");
    return false;
}

// Graph A.  KeyFrames 10 .. 17 and 20 .. 26 (store index = mnId - 10; 18, 19 unused).  The current map's chain 20 <- 21 <- ... <- 26,
// pCurrKF = 26: six window KeyFrames and 20 before them.  The merge map's chain 10 <- 11 <- 12 <- 13 <- 14, pMergeKF = 13, its
// mNextKF 14.  15, 16, 17 beside both.  Points (mnId 500 + p): 0 and 1 are seen by 26 AND 25, 2 .. 31 by 26 alone, so that the sort
// by observation count puts 0 and 1 last and the cut after 30 points leaves them out; 17 sees point 0 only (never gathered), 15
// sees point 2, 16 sees points 3 and 4; the fixed KeyFrame 10 sees point 2 at octave 11 (no edge) and points 3 and 4.
void graph_a(Graph& G) {
    for (int k = 11; k <= 16; k++) G.link(k, k - 1);       // 21 .. 26
    for (int k = 1; k <= 4; k++) G.link(k, k - 1);         // 11 .. 14
    G.store[3].mNextKF = G.kf[4];
    for (int p = 0; p < 32; p++) G.observe(16, p, 100.f + p, 50.f, p % 2 ? 90.f + p : -1.f, p % 4);
    G.observe(15, 0, 10, 11, -1, 0);
    G.observe(15, 1, 12, 13, -1, 0);
    G.observe(7, 0, 14, 15, -1, 0);
    G.observe(5, 2, 16, 17, -1, 1);
    G.observe(6, 3, 18, 19, -1, 2);
    G.observe(6, 4, 20, 21, 5, 3);
    G.observe(0, 2, 22, 23, -1, 11);
    G.observe(0, 3, 24, 25, -1, 0);
    G.observe(0, 4, 26, 27, -1, 0);
}

// Graph B: both pop_back arms.  The current chain is 24 <- 25 <- 26 alone (24 has no mPrevKF: it becomes the covisible KeyFrame
// and leaves the window); the merge chain is 10 <- 11 <- 12, pMergeKF = 12 (10 has no mPrevKF: it is walked into the window,
// becomes the fixed KeyFrame and leaves it).  Point 0 is seen by 26, 24, 12 and 10.
void graph_b(Graph& G) {
    G.link(16, 15); G.link(15, 14);
    G.link(2, 1); G.link(1, 0);
    G.observe(16, 0, 1, 2, -1, 0);
    G.observe(14, 0, 3, 4, -1, 0);
    G.observe(2, 0, 5, 6, -1, 0);
    G.observe(0, 0, 7, 8, -1, 0);
}

template <class B>
void lists_of(const B& b, std::vector<int>& ids, std::vector<int>& kinds, std::vector<int>& prev, std::vector<int>& cur, std::vector<int>& opt,
              std::vector<int>& cov, std::vector<int>& fixed) {
    for (const auto& k : b.kf_of_index) ids.push_back((int)k->mnId);
    for (const auto& k : b.kfs) kinds.push_back(k.kind);
    for (const auto& e : b.iedges) { prev.push_back(e.pre.kf_prev); cur.push_back(e.pre.kf_cur); }
    for (const auto& k : b.vpOptimizableKFs) opt.push_back((int)k->mnId);
    for (const auto& k : b.vpOptimizableCovKFs) cov.push_back((int)k->mnId);
    for (const auto& k : b.lFixedKeyFrames) fixed.push_back((int)k->mnId);
}

int hand_listed() {
    using ORB_SLAM3::msorb_host::GatherMergeInertialBA;
    using ORB_SLAM3::msorb_host::MergeInertialBA;
    bool ok = true;
    {
        Graph G(17, 32);
        graph_a(G);
        auto B = GatherMergeInertialBA(G.kf[16], G.kf[3]);
        if (!B.handled) { std::printf("graph A: not gathered\n"); return 4; }
        std::vector<int> ids, kinds, prev, cur, opt, cov, fixed, pts;
        lists_of(B, ids, kinds, prev, cur, opt, cov, fixed);
        for (const auto& p : B.lLocalMapPoints) pts.push_back((int)p->mnId - 500);
        ok &= same("window", opt, {26, 25, 24, 23, 22, 21, 13, 12, 11, 14});
        ok &= same("fixed", fixed, {10});
        ok &= cov.size() == 3 && cov[0] == 20 && cov[1] + cov[2] == 31 && (cov[1] == 15 || cov[1] == 16);   // 17 sees only a point behind the cut
        ok &= same("KeyFrame ids", ids, {10, 11, 12, 13, 14, 15, 16, 20, 21, 22, 23, 24, 25, 26});
        ok &= same("kinds", kinds, {1, 0, 0, 0, 0, 3, 3, 0, 0, 0, 0, 0, 0, 0});
        ok &= same("kf_prev", prev, {12, 11, 10, 9, 8, 7, 2, 1, 0, 3});
        ok &= same("kf_cur", cur, {13, 12, 11, 10, 9, 8, 3, 2, 1, 4});
        ok &= B.lLocalMapPoints.size() == 32 && pts[0] == 0 && pts[31] == 31;
        // the edges of points 0 .. 4 (26 = index 13, 25 = 12, 15 = 5, 16 = 6, 10 = 0); 17 is no vertex, octave 11 is no edge
        if (B.edge_kf.size() != 12 + 27 || B.edge_objects.size() != B.edge_kf.size()) { std::printf("graph A: %zu edges\n", B.edge_kf.size()); return 4; }
        std::vector<int> ekf(B.edge_kf.begin(), B.edge_kf.begin() + 12), ept(B.edge_point.begin(), B.edge_point.begin() + 12);
        ok &= same("edge_kf", ekf, {12, 13, 12, 13, 5, 13, 0, 6, 13, 0, 6, 13});
        ok &= same("edge_point", ept, {0, 0, 1, 1, 2, 2, 3, 3, 3, 4, 4, 4});
        ok &= B.u_right[10] == 5.f && B.inv_sigma2[10] == 0.125f && B.xy[20] == 20.f && B.u_right[0] == -1.f;
        ok &= B.iedges[0].huber == 1 && B.iedges[0].downweight == 0 && B.iedges[0].info_gyro[0] != 0 && B.new_bias.size() == 10;
        ok &= G.touched(false) == 0;
        B.restore_marks();
        ok &= G.touched(true) == 0;
        if (!ok) { std::printf("graph A differs\n"); return 4; }
    }
    {
        Graph G(17, 1);
        graph_b(G);
        auto B = GatherMergeInertialBA(G.kf[16], G.kf[2]);
        if (!B.handled) { std::printf("graph B: not gathered\n"); return 4; }
        std::vector<int> ids, kinds, prev, cur, opt, cov, fixed;
        lists_of(B, ids, kinds, prev, cur, opt, cov, fixed);
        ok &= same("window", opt, {26, 25, 12, 11});
        ok &= same("fixed", fixed, {10});
        ok &= same("covisible", cov, {24});
        ok &= same("KeyFrame ids", ids, {10, 11, 12, 24, 25, 26});
        ok &= same("kinds", kinds, {1, 0, 0, 0, 0, 0});
        ok &= same("kf_prev", prev, {4, 3, 1, 0});
        ok &= same("kf_cur", cur, {5, 4, 2, 1});
        ok &= same("edge_kf", B.edge_kf, {0, 2, 3, 5});
        ok &= G.store[0].mnBALocalForKF == 0 && G.store[0].mnBAFixedForKF == 26;   // :3969-3970
        if (!ok) { std::printf("graph B differs\n"); return 4; }
    }
    for (int variant = 0; variant < 6; variant++) {   // not handled: false, no setter called, the marks as they were
        Graph G(17, 32);
        graph_a(G);
        int curr = 16, merge = 3;
        if (variant == 0) G.store[6].mpCamera2 = &G.cam;                  // a covisible KeyFrame with a second camera
        if (variant == 1) G.store[13].mpImuPreintegrated = nullptr;       // a link without preintegration
        if (variant == 2) G.store[12].bImu = false;                       // ... or without bImu on one end
        if (variant == 3) G.store[5].mnId = 40;                           // a gathered KeyFrame above maxKFid
        if (variant == 4) { for (int k = 0; k < 17; k++) G.store[k].mnId = k < 3 ? k : 100 + k; curr = 2; merge = 0; }   // maxKFid <= 2
        if (variant == 5) merge = 14;                                     // pMergeKF inside the current window: one KeyFrame twice
        KeyFrameAndPose corr;
        bool stop = false;
        const bool ret = MergeInertialBA(G.kf[curr], G.kf[merge], &stop, &G.map, corr);
        if (ret || G.touched(true) != 0 || !corr.empty()) { std::printf("refusal %d: ret %d touched %d\n", variant, (int)ret, G.touched(true)); return 4; }
    }
    {   // the flag found set (:4312-4314): true; the marks and the SetNewBias of :4142 as the reference leaves them, nothing else
        Graph G(17, 32);
        graph_a(G);
        KeyFrameAndPose corr;
        bool stop = true;
        const bool ret = MergeInertialBA(G.kf[16], G.kf[3], &stop, &G.map, corr);
        int nb = 0;
        for (const auto& q : G.pre) nb += q.n_set_new_bias;
        if (!ret || nb != 10 || G.touched(false) != 10 || !corr.empty() || G.store[16].mnBALocalForKF != 26) {
            std::printf("flag set: ret %d SetNewBias %d touched %d\n", (int)ret, nb, G.touched(false));
            return 4;
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--hand")) return hand_listed();   // the hand-listed part alone: needs no device
    if (argc < 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int hd[6];
    if (std::fread(hd, 4, 6, in) != 6) return 2;
    const int K = hd[0], NI = hd[1], P = hd[2], E = hd[3], curr = hd[4], merge = hd[5];
    std::vector<msorb_iba_keyframe> kfs((size_t)K);
    std::vector<msorb_iba_inertial_edge> ie((size_t)NI);
    std::vector<float> C15(225 * (size_t)NI), pos(3 * (size_t)P), xy(2 * (size_t)E), ur((size_t)E), inv_level(8);
    std::vector<int> ekf((size_t)E), ept((size_t)E), octave((size_t)E);
    auto rd = [&](void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, in) == bytes; };
    if (!rd(kfs.data(), kfs.size() * sizeof(kfs[0])) || !rd(ie.data(), ie.size() * sizeof(ie[0])) || !rd(C15.data(), C15.size() * 4) ||
        !rd(pos.data(), pos.size() * 4) || !rd(ekf.data(), 4 * (size_t)E) || !rd(ept.data(), 4 * (size_t)E) ||
        !rd(xy.data(), 8 * (size_t)E) || !rd(ur.data(), 4 * (size_t)E) || !rd(octave.data(), 4 * (size_t)E) || !rd(inv_level.data(), 32))
        return 2;
    Graph G(K, P);
    for (int k = 0; k < K; k++) {
        KeyFrame& F = G.store[k];
        const msorb_iba_keyframe& s = kfs[k];
        F.mvInvLevelSigma2 = inv_level;
        F.fx = s.fx; F.fy = s.fy; F.cx = s.cx; F.cy = s.cy; F.mbf = s.mbf;
        F.bImu = s.kind != 2;
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) {
                F.Rwb(a, b) = (float)s.Rwb[3 * a + b]; F.Tcw.R(a, b) = (float)s.Rcw[3 * a + b];
                F.mImuCalib.mTcb.R(a, b) = (float)s.Rcb[3 * a + b];
            }
            F.twb(a) = (float)s.twb[a]; F.Tcw.t(a) = (float)s.tcw[a]; F.vel(a) = (float)s.v[a];
            F.mImuCalib.mTcb.t(a) = (float)s.tcb[a]; F.mImuCalib.mTbc.t(a) = (float)s.tbc[a];
        }
        F.bias = Bias((float)s.ba[0], (float)s.ba[1], (float)s.ba[2], (float)s.bg[0], (float)s.bg[1], (float)s.bg[2]);
    }
    for (int i = 0; i < NI; i++) {
        const msorb_inertial_edge& e = ie[i].pre;
        if (e.kf_prev < 0 || e.kf_prev >= K || e.kf_cur < 0 || e.kf_cur >= K) return 2;
        G.link(e.kf_cur, e.kf_prev);
        Preintegrated& q = G.pre[e.kf_cur];
        std::memcpy(q.dR.m, e.dR, 36); std::memcpy(q.JRg.m, e.JRg, 36); std::memcpy(q.JVg.m, e.JVg, 36); std::memcpy(q.JVa.m, e.JVa, 36);
        std::memcpy(q.JPg.m, e.JPg, 36); std::memcpy(q.JPa.m, e.JPa, 36); std::memcpy(q.dV.v, e.dV, 12); std::memcpy(q.dP.v, e.dP, 12);
        std::memcpy(q.C.m, C15.data() + 225 * (size_t)i, 900);
        q.b = Bias(e.bias[0], e.bias[1], e.bias[2], e.bias[3], e.bias[4], e.bias[5]);
        q.dT = e.dT;
    }
    for (int p = 0; p < P; p++) G.pstore[p].pos = Vec3f(pos[3 * (size_t)p], pos[3 * (size_t)p + 1], pos[3 * (size_t)p + 2]);
    for (int e = 0; e < E; e++) G.observe(ekf[e], ept[e], xy[2 * (size_t)e], xy[2 * (size_t)e + 1], ur[e], octave[e]);
    auto w_int = [&](int v) { std::fwrite(&v, 4, 1, out); };
    {   // the gathered problem
        auto B = ORB_SLAM3::msorb_host::GatherMergeInertialBA(G.kf[curr], G.kf[merge]);
        if (!B.handled) return 3;
        const int Kg = (int)B.kfs.size(), NIg = (int)B.iedges.size(), Pg = (int)B.lLocalMapPoints.size(), Eg = (int)B.edge_kf.size();
        w_int(1);
        w_int(0); w_int(Kg); w_int(NIg); w_int(Pg); w_int(Eg); w_int(-1); w_int(-1); w_int(0);
        std::fwrite(B.kfs.data(), sizeof(msorb_iba_keyframe), (size_t)Kg, out);
        std::fwrite(B.iedges.data(), sizeof(msorb_iba_inertial_edge), (size_t)NIg, out);
        std::fwrite(B.pos_w.data(), 4, 3 * (size_t)Pg, out);
        std::fwrite(B.edge_kf.data(), 4, (size_t)Eg, out);
        std::fwrite(B.edge_point.data(), 4, (size_t)Eg, out);
        std::fwrite(B.xy.data(), 4, 2 * (size_t)Eg, out);
        std::fwrite(B.u_right.data(), 4, (size_t)Eg, out);
        std::fwrite(B.inv_sigma2.data(), 4, (size_t)Eg, out);
        for (const auto& p : B.lLocalMapPoints) w_int((int)p->mnId - 500);
        B.restore_marks();
        if (G.touched(true) != 0) return 5;
    }
    std::fflush(out);
    KeyFrameAndPose corr;
    bool stop = false;
    const bool ret = ORB_SLAM3::msorb_host::MergeInertialBA(G.kf[curr], G.kf[merge], &stop, &G.map, corr);
    int n_new_bias = 0;
    for (const auto& q : G.pre) n_new_bias += q.n_set_new_bias;
    w_int(ret ? 1 : 0); w_int(G.map.change); w_int(n_new_bias);
    for (int k = 0; k < K; k++) {
        const KeyFrame& F = G.store[k];
        const auto at = corr.find(G.kf[k]);
        w_int(F.n_set_pose); w_int(F.n_set_velocity); w_int(F.n_set_bias); w_int(at != corr.end() ? 1 : 0);
        const float bias[6] = {F.bias.bax, F.bias.bay, F.bias.baz, F.bias.bwx, F.bias.bwy, F.bias.bwz};
        std::fwrite(F.Tcw.R.m, 4, 9, out); std::fwrite(F.Tcw.t.v, 4, 3, out); std::fwrite(F.vel.v, 4, 3, out); std::fwrite(bias, 4, 6, out);
        const Sim3 S = at != corr.end() ? at->second : Sim3();
        std::fwrite(S.r.m, 8, 9, out); std::fwrite(S.t.v, 8, 3, out); std::fwrite(&S.s, 8, 1, out);
    }
    for (int p = 0; p < P; p++) {
        w_int(G.pstore[p].n_set_pos); w_int(G.pstore[p].n_update);
        std::fwrite(G.pstore[p].pos.v, 4, 3, out);
    }
    for (int e = 0; e < E; e++) {
        const uint8_t still = G.pstore[ept[e]].obs.count(G.kf[ekf[e]]) ? 1 : 0;
        std::fwrite(&still, 1, 1, out);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
