// ms-slam_amd/host/Optimizer_device.h's FullInertialBA compiled against minimal stand-ins of KeyFrame / MapPoint / Map /
// IMU::Preintegrated / IMU::Bias / Sophus::SE3f that carry the member names Optimizer::FullInertialBA (src/Optimizer.cc:366-756) uses,
// linked to libmsorb.so through the C ABI.
//
//   dropin_full_inertial_ba in.bin out.bin
//   dropin_full_inertial_ba --hand            the hand-listed graph in both forms, nNonFixed < 3 and the refusals alone (no device)
// in : tests/full_inertial_ba_cases.py's write_dropin_scene: int32 init, iterations, loop_id, K, NI, P, E, float prior_g, prior_a, then
//      msorb_iba_keyframe [K], msorb_iba_inertial_edge [NI] (pre.kf_prev / kf_cur name the KeyFrames), the 15 x 15 float covariance of
//      every edge, pos_w [3 P], edge_kf [E], edge_point [E], xy [2 E], u_right [E], octave [E] (int32), mvInvLevelSigma2 [8].
//      KeyFrame k has mnId 10 + k, point p mnId 500 + p; every KeyFrame is free (bFixLocal = false, as at the call sites).
// out: the gathered problem in write_scenes' layout, then ret, change_index, n_SetNewBias on preintegrations (int32), per KeyFrame
//      { n_set_pose n_set_velocity n_set_bias mnBAGlobalForKF (int32) Rcw[9] tcw[3] v[3] bias[6] as the setters left them, then the
//      same sixteen + five floats of mTcwGBA / mVwbGBA / mBiasGBA }, per point { n_set_pos n_update mnBAGlobalForKF (int32) pos[3]
//      mPosGBA[3] }.
// Before that it runs the hand-listed checks; a mismatch prints its name and exits with 4.  Those checks call no library function.
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
struct SE3f {   // Sophus::SE3<float> as far as the routine uses it
    Mat3f R;
    Vec3f t;
    SE3f() {}
    SE3f(const Mat3f& R_, const Vec3f& t_) : R(R_), t(t_) {}
    Mat3f rotationMatrix() const { return R; }
    Vec3f translation() const { return t; }
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
    unsigned long max_id = 0;
    std::vector<KFPtr> kfs;                           // in the order GetAllKeyFrames() returns them
    std::vector<MPPtr> mps;
    std::mutex mMutexMapUpdate;
    unsigned long GetMaxKFid() const { return max_id; }
    std::vector<KFPtr> GetAllKeyFrames() const { return kfs; }
    std::vector<MPPtr> GetAllMapPoints() const { return mps; }
    void IncreaseChangeIndex() { change++; }
};
constexpr unsigned long kNoMark = 0;
struct MapPoint {
    unsigned long mnId = 0, mnBALocalForKF = kNoMark, mnBAGlobalForKF = 0;
    Vec3f mPosGBA;
    Map* map = nullptr;
    bool bad = false;
    float mTrackDepth = 20.f;
    Vec3f pos;
    std::map<KFPtr, std::tuple<int, int>> obs;
    int n_set_pos = 0, n_update = 0;
    bool isBad() const { return bad; }
    Map* GetMap() const { return map; }
    Vec3f GetWorldPos() const { return pos; }
    void SetWorldPos(const Vec3f& p) { pos = p; n_set_pos++; }
    void UpdateNormalAndDepth() { n_update++; }
    std::map<KFPtr, std::tuple<int, int>> GetObservations() const { return obs; }
    void EraseObservation(const KFPtr& k) { obs.erase(k); }
};
struct KeyFrame {
    unsigned long mnId = 0, mnBALocalForKF = kNoMark, mnBAFixedForKF = kNoMark, mnBAGlobalForKF = 0;
    SE3f mTcwGBA;
    Vec3f mVwbGBA;
    Bias mBiasGBA;
    Map* map = nullptr;
    bool bad = false, bImu = true;
    KFPtr mPrevKF;
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
    Map* GetMap() const { return map; }
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

// KeyFrames in ONE block, so that the order of a map keyed by shared_ptr<KeyFrame> (the order of a point's edges) is the order here
struct Graph {
    std::vector<KeyFrame> store;
    std::vector<Preintegrated> pre;
    std::vector<KFPtr> kf;
    std::vector<MPPtr> mp;
    Map map;
    Pinhole cam;
    explicit Graph(int K) : store(K), pre(K) {
        for (int k = 0; k < K; k++) {
            kf.push_back(KFPtr(&store[k], [](KeyFrame*) {}));
            store[k].mnId = 10 + k;
            store[k].map = &map;
            store[k].mpCamera = &cam;
            store[k].mvInvLevelSigma2 = {1.0f, 0.5f, 0.25f, 0.125f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.1f, 0.05f};
            for (int q = 0; q < 15; q++) pre[k].C.m[16 * q] = 1e-4f * (1 + q);   // an invertible covariance
        }
    }
    ~Graph() {   // the KeyFrames and the points hold each other
        for (auto& p : mp) p->obs.clear();
        for (auto& k : store) { k.mvpMapPoints.clear(); k.mPrevKF.reset(); }
    }
    void link(int k, int prev) { store[k].mPrevKF = kf[prev]; store[k].mpImuPreintegrated = &pre[k]; }
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
    int touched() const {   // setters, the GBA members' mark, SetNewBias on a preintegration, the change index
        int n = map.change;
        for (const auto& k : store) n += (k.mnBAGlobalForKF != 0) + k.n_set_pose + k.n_set_velocity + k.n_set_bias;
        for (const auto& q : pre) n += q.n_set_new_bias;
        for (const auto& p : mp) n += (p->mnBAGlobalForKF != 0) + p->n_set_pos + p->n_update;
        return n;
    }
    void publish() {   // the map's lists: the KeyFrames newest first, which is not the order of the unknowns
        map.kfs.assign(kf.rbegin(), kf.rend());
        map.mps = mp;
        map.max_id = store.empty() ? 0 : store.back().mnId;
    }
};

template <class T>
bool same(const char* name, const std::vector<T>& got, const std::vector<T>& want) {
    if (got == want) return true;
    std::printf("hand-listed graph: %s differs (%zu entries, %zu expected)\n", name, got.size(), want.size());
    return false;
}

// KeyFrames 10 .. 14 along one chain (11's mPrevKF is 10, ...), 14 without IMU and without mPrevKF; point 500 seen by 11, 13, 14;
// point 501 seen by 10, 12 and, at octave 11, by 13; point 502 without an observation
void hand_graph(Graph& G) {
    for (auto& k : G.store) { k.fx = k.fy = 700; k.cx = 600; k.cy = 180; k.mbf = 380; }
    G.link(1, 0); G.link(2, 1); G.link(3, 2);
    G.store[4].bImu = false;
    G.store[3].bias = Bias(0.1f, 0.2f, 0.3f, 0.01f, 0.02f, 0.03f);
    MPPtr p0 = G.add_point(500, 1, 2, 3), p1 = G.add_point(501, 4, 5, 6);
    G.add_point(502, 7, 8, 9);
    G.observe(3, p0, 301, 302, 290, 0);
    G.observe(3, p1, 311, 312, -1, 11);   // octave > 10: no edge (:586)
    G.observe(1, p0, 101, 102, -1, 1);
    G.observe(4, p0, 401, 402, -1, 2);
    G.observe(2, p1, 201, 202, -1, 3);
    G.observe(0, p1, 1, 2, 0.5f, 0);
    G.publish();
}

int hand_listed() {
    bool ok = true;
    for (int init = 0; init < 2; init++) {
        Graph G(5);
        hand_graph(G);
        // bFixLocal: 14 (no IMU) and 10 are fixed by their marks; maxKFid = 14
        G.store[4].mnBAFixedForKF = 14; G.store[0].mnBALocalForKF = 13;
        auto B = ORB_SLAM3::msorb_host::GatherFullInertialBA(&G.map, 7, true, init != 0, 2.f, 3.f);
        if (!B.handled || B.too_few) { std::printf("hand-listed graph %d: not gathered\n", init); return 4; }
        std::vector<int> kinds, ids, prev, cur, huber, down, nb;
        for (const auto& k : B.kfs) kinds.push_back(k.kind);
        for (const auto& k : B.kf_of_index) ids.push_back((int)k->mnId);
        for (const auto& e : B.iedges) { prev.push_back(e.pre.kf_prev); cur.push_back(e.pre.kf_cur); huber.push_back(e.huber); down.push_back(e.downweight); }
        for (const auto& k : B.new_bias) nb.push_back((int)k->mnId);
        ok &= same("KeyFrame ids", ids, {10, 11, 12, 13, 14});
        ok &= same("kinds", kinds, {1, 0, 0, 0, 2});
        ok &= same("kf_prev", prev, {2, 1, 0});       // the map lists its KeyFrames newest first: the reference's loop follows that
        ok &= same("kf_cur", cur, {3, 2, 1});
        ok &= same("huber", huber, {1, 1, 1});
        ok &= same("downweight", down, {0, 0, 0});
        ok &= same("SetNewBias", nb, {13, 12, 11});
        ok &= same("edge_kf", B.edge_kf, {1, 3, 4, 0, 2});
        ok &= same("edge_point", B.edge_point, {0, 0, 0, 1, 1});
        ok &= same("xy", B.xy, {101, 102, 301, 302, 401, 402, 1, 2, 201, 202});
        ok &= same("u_right", B.u_right, {-1, 290, -1, 0.5f, -1});
        ok &= same("inv_sigma2", B.inv_sigma2, {0.5f, 1.0f, 0.25f, 1.0f, 0.125f});
        ok &= same("pos_w", B.pos_w, {1, 2, 3, 4, 5, 6, 7, 8, 9});
        ok &= B.prob.init == init && B.prob.iterations == 7 && B.prob.prior_g == 2.f && B.prob.prior_a == 3.f;
        // pIncKF is the last KeyFrame of the map's list, 10: its biases (zero); the random-walk informations only without bInit
        ok &= B.prob.bg0[0] == 0 && B.prob.ba0[2] == 0;
        ok &= (B.iedges[0].info_gyro[0] != 0) == (init == 0);
        ok &= G.touched() == 0;
        if (!ok) { std::printf("hand-listed graph %d differs\n", init); return 4; }
    }
    {   // pIncKF: with the list reversed the last KeyFrame visited is 13
        Graph G(5);
        hand_graph(G);
        G.map.kfs.assign(G.kf.begin(), G.kf.end());
        G.store[4].mnBAFixedForKF = 14;
        auto B = ORB_SLAM3::msorb_host::GatherFullInertialBA(&G.map, 7, true, true, 2.f, 3.f);
        // 14 is the last one: no IMU, biases zero; drop it from the list and 13 is the last
        G.map.kfs.pop_back();
        G.map.max_id = 13;
        auto C = ORB_SLAM3::msorb_host::GatherFullInertialBA(&G.map, 7, false, true, 2.f, 3.f);
        ok &= B.handled && C.handled && C.kfs.size() == 4 && (float)C.prob.bg0[1] == 0.02f && (float)C.prob.ba0[2] == 0.3f;
        ok &= C.edge_kf == std::vector<int>({1, 3, 0, 2});   // the observation by 14 (mnId > maxKFid) is no edge
        if (!ok) { std::printf("pIncKF differs\n"); return 4; }
    }
    {   // nNonFixed < 3: true, nothing touched
        Graph G(5);
        hand_graph(G);
        G.store[4].mnBAFixedForKF = 14; G.store[0].mnBALocalForKF = 13; G.store[1].mnBALocalForKF = 14;
        const bool ret = ORB_SLAM3::msorb_host::FullInertialBA(&G.map, 7, true, 5ul);
        if (!ret || G.touched() != 0) { std::printf("nNonFixed < 3: ret %d touched %d\n", (int)ret, G.touched()); return 4; }
    }
    for (int variant = 0; variant < 4; variant++) {   // not handled: false, nothing touched
        Graph G(5);
        hand_graph(G);
        if (variant == 0) G.store[2].mpCamera2 = &G.cam;          // a KeyFrame with a second camera
        if (variant == 1) { /* KeyFrame 14 is free and has no IMU: bFixLocal = false */ }
        if (variant == 2) { G.store[4].bImu = true; G.store[4].mPrevKF = G.kf[2]; G.store[4].mpImuPreintegrated = &G.pre[4]; }   // 12 has two successors: no chain
        if (variant == 3) { G.store[4].bImu = true; G.store[2].mpImuPreintegrated = nullptr; }                                   // a link without preintegration
        bool stop = false;
        const bool ret = ORB_SLAM3::msorb_host::FullInertialBA(&G.map, 7, false, variant == 0 ? 0ul : 9ul, &stop, variant == 2);
        if (ret || G.touched() != 0) { std::printf("refusal %d: ret %d touched %d\n", variant, (int)ret, G.touched()); return 4; }
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
    int hd[7];
    float priors[2];
    if (std::fread(hd, 4, 7, in) != 7 || std::fread(priors, 4, 2, in) != 2) return 2;
    const int init = hd[0], iterations = hd[1], loop_id = hd[2], K = hd[3], NI = hd[4], P = hd[5], E = hd[6];
    std::vector<msorb_iba_keyframe> kfs((size_t)K);
    std::vector<msorb_iba_inertial_edge> ie((size_t)NI);
    std::vector<float> C15(225 * (size_t)NI), pos(3 * (size_t)P), xy(2 * (size_t)E), ur((size_t)E), inv_level(8);
    std::vector<int> ekf((size_t)E), ept((size_t)E), octave((size_t)E);
    auto rd = [&](void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, in) == bytes; };
    if (!rd(kfs.data(), kfs.size() * sizeof(kfs[0])) || !rd(ie.data(), ie.size() * sizeof(ie[0])) || !rd(C15.data(), C15.size() * 4) ||
        !rd(pos.data(), pos.size() * 4) || !rd(ekf.data(), 4 * (size_t)E) || !rd(ept.data(), 4 * (size_t)E) ||
        !rd(xy.data(), 8 * (size_t)E) || !rd(ur.data(), 4 * (size_t)E) || !rd(octave.data(), 4 * (size_t)E) || !rd(inv_level.data(), 32))
        return 2;
    Graph G(K);
    for (int k = 0; k < K; k++) {
        KeyFrame& F = G.store[k];
        const msorb_iba_keyframe& s = kfs[k];
        F.mvInvLevelSigma2 = inv_level;
        F.fx = s.fx; F.fy = s.fy; F.cx = s.cx; F.cy = s.cy; F.mbf = s.mbf;
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
    for (int p = 0; p < P; p++) G.add_point(500 + p, pos[3 * (size_t)p], pos[3 * (size_t)p + 1], pos[3 * (size_t)p + 2]);
    for (int e = 0; e < E; e++) G.observe(ekf[e], G.mp[ept[e]], xy[2 * (size_t)e], xy[2 * (size_t)e + 1], ur[e], octave[e]);
    G.publish();
    auto w_int = [&](int v) { std::fwrite(&v, 4, 1, out); };
    {   // the gathered problem
        auto B = ORB_SLAM3::msorb_host::GatherFullInertialBA(&G.map, iterations, false, init != 0, priors[0], priors[1]);
        if (!B.handled || B.too_few) return 3;
        const int Kg = (int)B.kfs.size(), NIg = (int)B.iedges.size(), Pg = (int)B.vpMPs.size(), Eg = (int)B.edge_kf.size();
        w_int(1);
        w_int(B.prob.init); w_int(B.prob.iterations); w_int(Kg); w_int(NIg); w_int(Pg); w_int(Eg); w_int(-1); w_int(-1);
        std::fwrite(&B.prob.prior_g, 1, 56, out);
        std::fwrite(B.kfs.data(), sizeof(msorb_iba_keyframe), (size_t)Kg, out);
        std::fwrite(B.iedges.data(), sizeof(msorb_iba_inertial_edge), (size_t)NIg, out);
        std::fwrite(B.pos_w.data(), 4, 3 * (size_t)Pg, out);
        std::fwrite(B.edge_kf.data(), 4, (size_t)Eg, out);
        std::fwrite(B.edge_point.data(), 4, (size_t)Eg, out);
        std::fwrite(B.xy.data(), 4, 2 * (size_t)Eg, out);
        std::fwrite(B.u_right.data(), 4, (size_t)Eg, out);
        std::fwrite(B.inv_sigma2.data(), 4, (size_t)Eg, out);
        if (G.touched() != 0) return 5;
    }
    bool stop = false;
    const bool ret = ORB_SLAM3::msorb_host::FullInertialBA(&G.map, iterations, false, (unsigned long)loop_id, &stop, init != 0, priors[0], priors[1]);
    int n_new_bias = 0;
    for (const auto& q : G.pre) n_new_bias += q.n_set_new_bias;
    w_int(ret ? 1 : 0); w_int(G.map.change); w_int(n_new_bias);
    for (int k = 0; k < K; k++) {
        const KeyFrame& F = G.store[k];
        w_int(F.n_set_pose); w_int(F.n_set_velocity); w_int(F.n_set_bias); w_int((int)F.mnBAGlobalForKF);
        const float bias[6] = {F.bias.bax, F.bias.bay, F.bias.baz, F.bias.bwx, F.bias.bwy, F.bias.bwz};
        const float gba[6] = {F.mBiasGBA.bax, F.mBiasGBA.bay, F.mBiasGBA.baz, F.mBiasGBA.bwx, F.mBiasGBA.bwy, F.mBiasGBA.bwz};
        std::fwrite(F.Tcw.R.m, 4, 9, out); std::fwrite(F.Tcw.t.v, 4, 3, out); std::fwrite(F.vel.v, 4, 3, out); std::fwrite(bias, 4, 6, out);
        std::fwrite(F.mTcwGBA.R.m, 4, 9, out); std::fwrite(F.mTcwGBA.t.v, 4, 3, out); std::fwrite(F.mVwbGBA.v, 4, 3, out); std::fwrite(gba, 4, 6, out);
    }
    for (int p = 0; p < P; p++) {
        w_int(G.mp[p]->n_set_pos); w_int(G.mp[p]->n_update); w_int((int)G.mp[p]->mnBAGlobalForKF);
        std::fwrite(G.mp[p]->pos.v, 4, 3, out);
        std::fwrite(G.mp[p]->mPosGBA.v, 4, 3, out);
    }
    std::fclose(in);
    std::fclose(out);
    return 0;
}
