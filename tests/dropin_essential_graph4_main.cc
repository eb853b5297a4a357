// ms-slam_amd/host/Optimizer_device.h's OptimizeEssentialGraph4DoF compiled against minimal stand-ins of KeyFrame / MapPoint / Map /
// Sophus::SE3f / g2o::Sim3 that carry the member names Optimizer::OptimizeEssentialGraph4DoF (src/Optimizer.cc:5174-5458) uses,
// linked to libmsorb.so through the C ABI.  The program makes its own map of twelve KeyFrames 0..11 (1 is the loop KeyFrame and the
// only fixed vertex; 11 closes the loop with it) and lists beside it the edges every live arm has to give: the loop connections
// with the weight gate and its pCurKF / pLoopKF exemption, the mPrevKF arm, an older loop edge, the covisibility arm with its
// exclusions (mPrevKF, mNextKF, a child, a loop edge, a pair already in sInsertedEdges, a bad, a null and a younger neighbour).
// The spanning-tree arm is dead in this fork: every KeyFrame has a parent, and a parent that is neither mPrevKF nor a covisible
// gets no edge.  KeyFrames 10 and 11 are in CorrectedSim3 (with a scale, which the vertex drops) and are built by
// ImuCamPose(Rwc, twc, pKF); the others by ImuCamPose(pKF) from four floats.  Every check compares what the routine did to the map
// with what msorb_essential_graph4 returns for the hand-listed arrays: SetPose and the point correction byte for byte, a bad
// point untouched.  Then `false` with nothing touched: a bad KeyFrame in the map, an id above GetMaxKFid(), more free KeyFrames
// than the capacity; and an mPrevKF without a vertex whose edge is not added while the rest is optimised.
// Prints "ok" and exits with 0, or names the check that failed and exits with 1.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <vector>

#include "Optimizer_device.h"

namespace {

using msorb::sim3opt::Sim3;
using msorb::sim3opt::sim3_inverse;
using msorb::sim3opt::sim3_map;
using msorb::sim3opt::sim3_mul;

template <class T>
struct Vec3 {
    T v[3];
    Vec3() : v{0, 0, 0} {}
    Vec3(T x, T y, T z) : v{x, y, z} {}
    T operator()(int i) const { return v[i]; }
};
template <class T>
struct Quat {
    T w_, x_, y_, z_;
    Quat() : w_(1), x_(0), y_(0), z_(0) {}
    Quat(T w, T x, T y, T z) : w_(w), x_(x), y_(y), z_(z) {}   // Eigen's argument order
    T x() const { return x_; }
    T y() const { return y_; }
    T z() const { return z_; }
    T w() const { return w_; }
};
typedef Vec3<float> Vec3f;
struct Mat3f {
    float m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    float operator()(int r, int c) const { return m[3 * r + c]; }
};
struct SE3f {   // Sophus::SE3<float> as far as the routine uses it (no normalisation here: what SetPose receives is what is stored)
    Quat<float> q;
    Vec3f t;
    SE3f() {}
    SE3f(const Quat<float>& q_, const Vec3f& t_) : q(q_), t(t_) {}
    const Quat<float>& unit_quaternion() const { return q; }
    const Vec3f& translation() const { return t; }
    Mat3f rotationMatrix() const {
        Mat3f R;
        const float x = q.x(), y = q.y(), z = q.z(), w = q.w();
        const float r[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                            2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
        std::memcpy(R.m, r, sizeof r);
        return R;
    }
};
struct G2oSim3 {   // g2o::Sim3's getters
    Quat<double> r;
    Vec3<double> t;
    double s = 1;
    const Quat<double>& rotation() const { return r; }
    const Vec3<double>& translation() const { return t; }
    double scale() const { return s; }
};
struct KeyFrame;
struct MapPoint;
typedef std::shared_ptr<KeyFrame> KFPtr;
typedef std::shared_ptr<MapPoint> MPPtr;
struct Map {
    unsigned long max_id = 0;
    std::vector<KFPtr> all_kfs;
    std::vector<MPPtr> all_mps;
    std::mutex mMutexMapUpdate;
    int n_change = 0;
    unsigned long GetMaxKFid() const { return max_id; }
    std::vector<KFPtr> GetAllKeyFrames() const { return all_kfs; }
    std::vector<MPPtr> GetAllMapPoints() const { return all_mps; }
    void IncreaseChangeIndex() { n_change++; }
};
struct MapPoint {
    bool bad = false;
    Vec3f pos;
    KFPtr ref;
    int n_set = 0, n_update = 0;
    bool isBad() const { return bad; }
    Vec3f GetWorldPos() const { return pos; }
    void SetWorldPos(const Vec3f& p) { pos = p; n_set++; }
    void UpdateNormalAndDepth() { n_update++; }
    KFPtr GetReferenceKeyFrame() const { return ref; }
};
struct ImuCalib {
    SE3f mTcb;
};
struct KeyFrame {
    unsigned long mnId = 0;
    bool bad = false;
    SE3f Tcw;
    Mat3f Rwb;    // the IMU pose is kept beside the camera pose, as the KeyFrame keeps it: four floats of their own
    Vec3f twb;
    ImuCalib mImuCalib;
    KFPtr parent, mPrevKF, mNextKF;
    std::set<KFPtr> children, loop_edges;
    std::vector<std::pair<int, KFPtr>> covisibles;   // by weight, descending
    int n_set_pose = 0;
    bool isBad() const { return bad; }
    SE3f GetPose() const { return Tcw; }
    Mat3f GetRotation() const { return Tcw.rotationMatrix(); }
    Vec3f GetTranslation() const { return Tcw.t; }
    Mat3f GetImuRotation() const { return Rwb; }
    Vec3f GetImuPosition() const { return twb; }
    void SetPose(const SE3f& T) { Tcw = T; n_set_pose++; }
    KFPtr GetParent() const { return parent; }
    bool hasChild(const KFPtr& p) const { return children.count(p) != 0; }
    std::set<KFPtr> GetLoopEdges() const { return loop_edges; }
    int GetWeight(const KFPtr& p) const {
        for (const auto& c : covisibles)
            if (c.second == p) return c.first;
        return 0;
    }
    std::vector<KFPtr> GetCovisiblesByWeight(int w) const {
        std::vector<KFPtr> out;
        for (const auto& c : covisibles)
            if (c.first >= w) out.push_back(c.second);
        return out;
    }
};
typedef std::map<KFPtr, G2oSim3> KeyFrameAndPose;   // (the reference's has an aligned allocator besides)

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("line %d: %s does not hold\n", __LINE__, #c); \
            return 1;                                                 \
        }                                                             \
    } while (0)

unsigned rnd(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
float uni(unsigned& s) { return (float)(rnd(s) % 20001) / 10000.0f - 1.0f; }

// KeyFrames in ONE block, so that containers keyed by shared_ptr<KeyFrame> walk them in the order of their ids
struct World {
    std::vector<KeyFrame> store;
    std::vector<KFPtr> kf;
    Map map;
    explicit World(int n) : store((size_t)n) {
        unsigned seed = 4711;
        const SE3f Tcb(Quat<float>(0.5f, -0.5f, 0.5f, -0.5f), Vec3f(0.05f, -0.02f, 0.11f));   // an axis swap and a lever arm
        for (int k = 0; k < n; k++) {
            kf.push_back(KFPtr(&store[k], [](KeyFrame*) {}));
            KeyFrame& f = store[k];
            f.mnId = (unsigned long)k;
            f.mImuCalib.mTcb = Tcb;
            const float ax = 0.02f * uni(seed), ay = 0.03f * uni(seed) + 0.02f * k, az = 0.02f * uni(seed);
            const float w = std::sqrt(1 - ax * ax - ay * ay - az * az);   // (not normalised to the last bit)
            f.Tcw = SE3f(Quat<float>(w, ax, ay, az), Vec3f(0.9f * k + 0.1f * uni(seed), 0.1f * uni(seed), 0.2f * uni(seed)));
            // the body pose of that camera pose, in float: Rwb = Rcw^T Rcb, twb = Rcw^T (tcb - tcw)
            const Mat3f Rcw = f.Tcw.rotationMatrix(), Rcb = Tcb.rotationMatrix();
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) f.Rwb.m[3 * r + c] = Rcw(0, r) * Rcb(0, c) + Rcw(1, r) * Rcb(1, c) + Rcw(2, r) * Rcb(2, c);
                f.twb.v[r] = Rcw(0, r) * (Tcb.t(0) - f.Tcw.t(0)) + Rcw(1, r) * (Tcb.t(1) - f.Tcw.t(1)) + Rcw(2, r) * (Tcb.t(2) - f.Tcw.t(2));
            }
            if (k > 0) { f.mPrevKF = kf[k - 1]; store[k - 1].mNextKF = kf[k]; }
            map.all_kfs.push_back(kf[k]);
        }
        // the spanning tree is NOT the temporal chain here: k's parent is k - 3 (0, 1, 2 hang off 0), so a parent is never mPrevKF
        for (int k = 1; k < n; k++) { store[k].parent = kf[std::max(0, k - 3)]; store[std::max(0, k - 3)].children.insert(kf[k]); }
        map.max_id = (unsigned long)n - 1;
    }
};

Sim3 sim3_of_pose(const SE3f& T) {   // Tcw.cast<double>() (Sophus normalises again), then g2o::Sim3(q, t, 1.0)
    const double x = T.q.x(), y = T.q.y(), z = T.q.z(), w = T.q.w();
    const double len = std::sqrt(((x * x + y * y) + z * z) + w * w);
    return Sim3{x / len, y / len, z / len, w / len, (double)T.t(0), (double)T.t(1), (double)T.t(2), 1.0};
}
G2oSim3 g2o_of(const Sim3& S) {
    G2oSim3 g;
    g.r = Quat<double>(S.qw, S.qx, S.qy, S.qz);
    g.t = Vec3<double>(S.tx, S.ty, S.tz);
    g.s = S.s;
    return g;
}
bool same_pose(const SE3f& a, const SE3f& b) { return std::memcmp(&a.q, &b.q, sizeof a.q) == 0 && std::memcmp(&a.t, &b.t, sizeof a.t) == 0; }

struct Snapshot {
    std::vector<SE3f> poses;
    std::vector<Vec3f> points;
    explicit Snapshot(const World& W) {
        for (const auto& f : W.store) poses.push_back(f.Tcw);
        for (const auto& m : W.map.all_mps) points.push_back(m->pos);
    }
    bool untouched(const World& W) const {
        for (size_t k = 0; k < W.store.size(); k++)
            if (!same_pose(W.store[k].Tcw, poses[k]) || W.store[k].n_set_pose) return false;
        for (size_t p = 0; p < points.size(); p++)
            if (std::memcmp(&W.map.all_mps[p]->pos, &points[p], sizeof(Vec3f)) || W.map.all_mps[p]->n_set) return false;
        return W.map.n_change == 0;
    }
};

int loop_closing() {
    World W(12);
    auto& kf = W.kf;
    auto& st = W.store;
    const KFPtr pCurKF = kf[11], pLoopKF = kf[1];
    KeyFrame outsider;   // a bad neighbour that is no longer in the map
    outsider.mnId = 3; outsider.bad = true;
    const KFPtr pBad(&outsider, [](KeyFrame*) {});
    auto link = [&](int a, int b, int w) { st[a].covisibles.push_back({w, kf[b]}); st[b].covisibles.push_back({w, kf[a]}); };
    for (int k = 2; k < 12; k++) link(k, k - 2, 120);            // the covisibility arm: (k, k - 2), except where excluded below
    for (int k = 1; k < 12; k++) link(k, k - 1, 200);            // mPrevKF / mNextKF: skipped there
    link(9, 6, 150);                                             // 6 is 9's PARENT: pParentKF is NULL, so the covisibility arm takes it
    link(8, 4, 110);                                             // a plain covisible beside the regular one
    st[10].children.insert(kf[5]);                               // a child OLDER than its KeyFrame: (10, 5) is skipped by hasChild
    link(10, 5, 140);
    link(11, 2, 130);                                            // passes the loop gate, and is then in sInsertedEdges
    link(11, 3, 10);                                             // gated: 10 < 100 * 0.3
    link(11, 1, 5);                                              // below the gate, but pCurKF -> pLoopKF is exempt
    link(10, 1, 35);                                             // passes the gate, below minFeat for the covisibility arm
    link(7, 3, 160);                                             // also a loop edge: skipped by sLoopEdges.count
    st[8].covisibles.push_back({300, pBad});                     // a bad neighbour
    st[8].covisibles.push_back({250, KFPtr()});                  // and a null one
    for (auto& f : st) std::stable_sort(f.covisibles.begin(), f.covisibles.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    st[7].loop_edges.insert(kf[3]); st[3].loop_edges.insert(kf[7]);   // an older loop: the arm takes (7 -> 3) only
    KeyFrame gone;       // a KeyFrame that left the map but is still an mPrevKF: no vertex, its edge is not added
    gone.mnId = 12;
    const KFPtr pGone(&gone, [](KeyFrame*) {});
    W.map.max_id = 13;
    st[0].mPrevKF = pGone;
    std::map<KFPtr, std::set<KFPtr>> LoopConnections;
    LoopConnections[kf[11]] = {kf[1], kf[2], kf[3]};
    LoopConnections[kf[10]] = {kf[1]};
    KeyFrameAndPose Corrected, NonCorrected;
    const double correction[7] = {0.0, 0.0, 0.04, 0.3, -0.1, 0.05, 0.03};   // with a scale: the 4-DoF vertex drops it
    const Sim3 fix = msorb::sim3opt::sim3_exp(correction);
    for (int k : {10, 11}) {
        NonCorrected[kf[k]] = g2o_of(sim3_of_pose(st[k].Tcw));
        Corrected[kf[k]] = g2o_of(sim3_mul(sim3_of_pose(st[k].Tcw), fix));
    }
    unsigned seed = 99;
    for (int p = 0; p < 30; p++) {
        MPPtr m = std::make_shared<MapPoint>();
        m->pos = Vec3f(10 * uni(seed), 2 * uni(seed), 8 + 6 * uni(seed));
        m->ref = kf[p % 12];
        if (p == 7) m->bad = true;
        W.map.all_mps.push_back(m);
    }
    // ---- the arrays the routine has to gather, listed by hand
    const Sim3 identity{0, 0, 0, 1, 0, 0, 0, 1};
    std::vector<Sim3> vScw(14, identity);
    std::vector<msorb_eg4_vertex> vertices(12);
    for (int k = 0; k < 12; k++) {
        msorb_eg4_vertex& v = vertices[k];
        std::memset(&v, 0, sizeof v);
        const Mat3f Rcb = st[k].mImuCalib.mTcb.rotationMatrix();
        for (int q = 0; q < 9; q++) v.Rcb[q] = Rcb.m[q];
        for (int q = 0; q < 3; q++) v.tcb[q] = st[k].mImuCalib.mTcb.t(q);
        if (k >= 10) {   // ImuCamPose(Rwc, twc, pKF)
            vScw[k] = ORB_SLAM3::msorb_host::EgSim3(Corrected.find(kf[k])->second);
            const Sim3 Swc = sim3_inverse(vScw[k]);
            double Rwc[9];
            ORB_SLAM3::msorb_host::EgRotationOfQuaternion(Swc, Rwc);
            const double twc[3] = {Swc.tx, Swc.ty, Swc.tz};
            for (int r = 0; r < 3; r++) {
                v.twb[r] = ((Rwc[3 * r] * v.tcb[0] + Rwc[3 * r + 1] * v.tcb[1]) + Rwc[3 * r + 2] * v.tcb[2]) + twc[r];
                for (int c = 0; c < 3; c++) {
                    v.Rwb[3 * r + c] = (Rwc[3 * r] * v.Rcb[c] + Rwc[3 * r + 1] * v.Rcb[3 + c]) + Rwc[3 * r + 2] * v.Rcb[6 + c];
                    v.Rcw[3 * r + c] = Rwc[3 * c + r];
                }
            }
            for (int r = 0; r < 3; r++) v.tcw[r] = -((v.Rcw[3 * r] * twc[0] + v.Rcw[3 * r + 1] * twc[1]) + v.Rcw[3 * r + 2] * twc[2]);
        } else {         // ImuCamPose(pKF)
            vScw[k] = sim3_of_pose(st[k].Tcw);
            const Mat3f Rcw = st[k].Tcw.rotationMatrix();
            for (int q = 0; q < 9; q++) { v.Rcw[q] = Rcw.m[q]; v.Rwb[q] = st[k].Rwb.m[q]; }
            for (int q = 0; q < 3; q++) { v.tcw[q] = st[k].Tcw.t(q); v.twb[q] = st[k].twb(q); }
        }
        v.fixed = k == 1;
    }
    auto non_corrected = [&](int k) { return (k == 10 || k == 11) ? sim3_of_pose(st[k].Tcw) : vScw[k]; };
    std::vector<int> v0, v1;
    std::vector<double> meas;
    auto edge = [&](int i, int j, const Sim3& Siw, const Sim3& Sjw) {
        v0.push_back(i); v1.push_back(j);
        const Sim3 Sij = sim3_mul(Siw, sim3_inverse(Sjw));
        double m[12];
        ORB_SLAM3::msorb_host::EgRotationOfQuaternion(Sij, m);
        m[9] = Sij.tx; m[10] = Sij.ty; m[11] = Sij.tz;
        meas.insert(meas.end(), m, m + 12);
    };
    // the loop connections, in the map's order (10 before 11), with the CORRECTED poses: (10, 1) passes the gate with 35;
    // (11, 1) is exempt; (11, 2) passes with 130; (11, 3) is gated
    edge(10, 1, vScw[10], vScw[1]);
    edge(11, 1, vScw[11], vScw[1]);
    edge(11, 2, vScw[11], vScw[2]);
    // per KeyFrame: mPrevKF, older loop edges, covisibles (weight descending, then insertion order)
    for (int k = 0; k < 12; k++) {
        if (k > 0) edge(k, k - 1, non_corrected(k), non_corrected(k - 1));     // (0's mPrevKF has no vertex)
        if (k == 7) edge(7, 3, non_corrected(7), non_corrected(3));           // the loop edge, once
        if (k == 9) edge(9, 6, non_corrected(9), non_corrected(6));           // weight 150: its parent, through the covisibility arm
        // (10, 5): a child; (11, 2): in sInsertedEdges; (7, 3) again: a loop edge; (8, bad), (8, null): skipped
        if (k >= 2 && k != 11) edge(k, k - 2, non_corrected(k), non_corrected(k - 2));   // weight 120
        if (k == 11) edge(11, 9, non_corrected(11), non_corrected(9));
        if (k == 8) edge(8, 4, non_corrected(8), non_corrected(4));           // weight 110
    }
    std::vector<double> poses(12 * 12);
    msorb_eg4_result r;
    CHECK(msorb_essential_graph4(0, 12, vertices.data(), (int)v0.size(), v0.data(), v1.data(), meas.data(), 20, poses.data(), &r, nullptr) == MSORB_OK);
    CHECK(r.iterations > 0 && r.chi2_final < r.chi2_initial && r.lambda_initial > 0);
    std::vector<Vec3f> before;
    for (const auto& m : W.map.all_mps) before.push_back(m->pos);
    CHECK(ORB_SLAM3::msorb_host::OptimizeEssentialGraph4DoF(&W.map, pLoopKF, pCurKF, NonCorrected, Corrected, LoopConnections));
    CHECK(W.map.n_change == 1);
    std::vector<Sim3> vCorrectedSwc(14, identity);
    int moved = 0;
    for (int k = 0; k < 12; k++) {
        const double* o = &poses[12 * (size_t)k];
        double q[4], back[9];
        ORB_SLAM3::msorb_host::EgQuaternionOfRotation(o, q);
        const Sim3 S{q[0], q[1], q[2], q[3], o[9], o[10], o[11], 1.0};
        ORB_SLAM3::msorb_host::EgRotationOfQuaternion(S, back);            // the quaternion is the matrix's
        for (int e = 0; e < 9; e++) CHECK(std::fabs(back[e] - o[e]) < 1e-5);   // (Rcw comes from float poses: orthonormal to 1e-7)
        vCorrectedSwc[k] = sim3_inverse(S);
        const double len = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
        const SE3f want(Quat<float>((float)(q[3] / len), (float)(q[0] / len), (float)(q[1] / len), (float)(q[2] / len)),
                        Vec3f((float)o[9], (float)o[10], (float)o[11]));
        CHECK(st[k].n_set_pose == 1 && same_pose(st[k].Tcw, want));
        if (k != 1 && std::fabs(o[9] - vertices[k].tcw[0]) > 1e-6) moved++;
    }
    CHECK(moved >= 8);   // the correction of 0.3 at the loop's end is spread over the chain
    for (int p = 0; p < 30; p++) {
        const MapPoint& m = *W.map.all_mps[p];
        if (p == 7) { CHECK(m.n_set == 0 && m.n_update == 0 && std::memcmp(&m.pos, &before[p], sizeof(Vec3f)) == 0); continue; }
        const int ref = p % 12;
        double x, y, z, cx, cy, cz;
        sim3_map(vScw[ref], (double)before[p](0), (double)before[p](1), (double)before[p](2), x, y, z);
        sim3_map(vCorrectedSwc[ref], x, y, z, cx, cy, cz);
        const Vec3f want((float)cx, (float)cy, (float)cz);
        CHECK(m.n_set == 1 && m.n_update == 1 && std::memcmp(&m.pos, &want, sizeof want) == 0);
    }
    return 0;
}

int refusals() {
    {   // a bad KeyFrame in the map
        World W(6);
        W.map.all_mps.push_back(std::make_shared<MapPoint>());
        W.map.all_mps[0]->ref = W.kf[2];
        W.store[4].bad = true;
        const Snapshot snap(W);
        KeyFrameAndPose none;
        std::map<KFPtr, std::set<KFPtr>> lc;
        CHECK(!ORB_SLAM3::msorb_host::OptimizeEssentialGraph4DoF(&W.map, W.kf[0], W.kf[5], none, none, lc));
        CHECK(snap.untouched(W));
    }
    {   // an id above GetMaxKFid()
        World W(6);
        W.map.all_mps.push_back(std::make_shared<MapPoint>());
        W.map.all_mps[0]->ref = W.kf[2];
        W.map.max_id = 4;
        const Snapshot snap(W);
        KeyFrameAndPose none;
        std::map<KFPtr, std::set<KFPtr>> lc;
        CHECK(!ORB_SLAM3::msorb_host::OptimizeEssentialGraph4DoF(&W.map, W.kf[0], W.kf[5], none, none, lc));
        CHECK(snap.untouched(W));
    }
    {   // more free KeyFrames than the capacity
        const int n = msorb_essential_graph4_capacity() + 2;
        World W(n);
        W.map.all_mps.push_back(std::make_shared<MapPoint>());
        W.map.all_mps[0]->ref = W.kf[2];
        const Snapshot snap(W);
        KeyFrameAndPose none;
        std::map<KFPtr, std::set<KFPtr>> lc;
        CHECK(!ORB_SLAM3::msorb_host::OptimizeEssentialGraph4DoF(&W.map, W.kf[0], W.kf[n - 1], none, none, lc));
        CHECK(snap.untouched(W));
    }
    return 0;
}

}  // namespace

int main() {
    if (loop_closing()) return 1;
    if (refusals()) return 1;
    std::printf("ok\n");
    return 0;
}
