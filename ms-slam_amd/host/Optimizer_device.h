// Optimizer::PoseOptimization (src/Optimizer.cc:759-1037), LocalBundleAdjustment, BundleAdjustment / GlobalBundleAdjustemnt and the two OptimizeSim3 (further down), each on
// its device entry of libmsorb.  First PoseOptimization (msorb_pose_optimization_batch /
// msorb_frame_pose_optimization), written against the reference's own types by name (a template: this header compiles inside
// MS-SLAM, where Frame / MapPoint are the real classes, and in tests/dropin_poseopt_main.cc, where they are minimal stand-ins
// with the same member names).
//
//   int ORB_SLAM3::msorb_host::PoseOptimization(Frame* pFrame)                              the reference's signature
//   int ORB_SLAM3::msorb_host::PoseOptimization(Frame* pFrame, msorb_frame* resident)       keypoints already on a handle
//
// Effects as the reference's: mvbOutlier of every entry with a usable map point, SetPose with the narrowed estimate, the
// return value nInitialCorrespondences - nBad (0, and no SetPose, below three correspondences, :936-937).
//
// What runs where.  The gathering loop (:799-934, under MapPoint::mGlobalMutex) stays on the host: it reads the map points.
// The four rounds, every Levenberg step and the classifications are one device launch.
//
// Scope: pinhole mono / stereo frames.  A frame with a second camera (pFrame->mpCamera2, the arm :870-931) is NOT handled:
// the function returns -1 without touching the frame and the caller keeps Optimizer::PoseOptimization for it, as for the
// inertial variants.  The camera is read from pFrame->fx, fy, cx, cy, mbf, which for Pinhole are the values pCamera->project
// uses (mvParameters[0..3]).
//
// `resident`: a handle whose keypoint table holds THIS frame's mvKeysUn, mvuRight and octaves (DeviceFrame::Upload /
// ExtractStereoFrame of ORBmatcher_device.h).  The handle is filled from mvKeys by the device front-end, so this form is valid
// when mvKeysUn == mvKeys, i.e. for rectified input (Frame::UndistortKeyPoints with mDistCoef(0) == 0, Frame.cc:679-685).  Then
// only the indices of the matched keypoints and their points' positions go up.  Without it everything goes up as flat arrays.
#ifndef MSORB_OPTIMIZER_DEVICE_H
#define MSORB_OPTIMIZER_DEVICE_H

#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <tuple>
#include <utility>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "msorb.h"

namespace ORB_SLAM3 {
namespace msorb_host {
#ifndef MSORB_HOST_FAIL_CALL
#define MSORB_HOST_FAIL_CALL
// a failed call of the C ABI: the application's fatal-error callback first (msorb_set_fatal_callback), then std::runtime_error
[[noreturn]] inline void fail_call(const char* what) {
    const std::string msg = std::string(what) + ": " + msorb_last_error();
    msorb_notify_fatal(MSORB_E_HIP, msg.c_str());
    throw std::runtime_error(msg);
}
#endif

template <class FrameT>
int PoseOptimization(FrameT* pFrame, msorb_frame* resident, int device = 0) {
    if (pFrame->mpCamera2) return -1;   // the two-camera arm stays the reference's
    typedef typename std::decay<decltype(*pFrame->mvpMapPoints[0])>::type MapPointT;
    const int N = pFrame->N;
    // per calling thread, kept between frames
    static thread_local std::vector<uint8_t> has, out;
    static thread_local std::vector<float> pos, xy, ur, inv;
    static thread_local std::vector<int> index;
    has.assign((size_t)N, 0);
    pos.resize(3 * (size_t)N);
    index.clear();
    int nInitialCorrespondences = 0;
    {
        std::unique_lock<std::mutex> lock(MapPointT::mGlobalMutex);   // :800
        for (int i = 0; i < N; i++) {
            const auto pMP = pFrame->mvpMapPoints[i];
            if (pMP && !pMP->isBad()) {        // :804
                nInitialCorrespondences++;     // :809, :836
                pFrame->mvbOutlier[i] = false;  // :810, :837
                const auto Xw = pMP->GetWorldPos();   // :828, :861
                has[i] = 1;
                pos[3 * (size_t)i] = Xw(0); pos[3 * (size_t)i + 1] = Xw(1); pos[3 * (size_t)i + 2] = Xw(2);
                index.push_back(i);
            }
        }
    }
    if (nInitialCorrespondences < 3) return 0;   // :936-937
    const auto Tcw = pFrame->GetPose();          // :774
    typedef typename std::decay<decltype(Tcw)>::type SE3T;
    typedef typename std::decay<decltype(Tcw.unit_quaternion())>::type QuatT;
    typedef typename std::decay<decltype(Tcw.translation())>::type VecT;
    msorb_pose_problem p;
    const auto& q = Tcw.unit_quaternion();
    const auto& t = Tcw.translation();
    p.q[0] = q.x(); p.q[1] = q.y(); p.q[2] = q.z(); p.q[3] = q.w();
    p.t[0] = t(0); p.t[1] = t(1); p.t[2] = t(2);
    p.fx = pFrame->fx; p.fy = pFrame->fy; p.cx = pFrame->cx; p.cy = pFrame->cy; p.mbf = pFrame->mbf;   // :856-860
    p.n = nInitialCorrespondences;
    msorb_pose_result r;
    out.assign((size_t)N, 0);
    if (resident) {
        if (msorb_frame_pose_optimization(resident, &p, has.data(), pos.data(), pFrame->mvInvLevelSigma2.data(),
                                          (int)pFrame->mvInvLevelSigma2.size(), out.data(), &r) != MSORB_OK)
            fail_call("msorb_frame_pose_optimization");
        for (int i : index) pFrame->mvbOutlier[i] = out[i] != 0;
    } else {
        const size_t m = index.size();
        xy.resize(2 * m); ur.resize(m); inv.resize(m);
        for (size_t k = 0; k < m; k++) {
            const int i = index[k];
            const auto& kpUn = pFrame->mvKeysUn[i];                  // :813, :840
            xy[2 * k] = kpUn.pt.x; xy[2 * k + 1] = kpUn.pt.y;
            ur[k] = pFrame->mvuRight[i];                             // :808, :841
            inv[k] = pFrame->mvInvLevelSigma2[kpUn.octave];          // :820, :848
            pos[3 * k] = pos[3 * (size_t)i]; pos[3 * k + 1] = pos[3 * (size_t)i + 1]; pos[3 * k + 2] = pos[3 * (size_t)i + 2];   // (k <= i)
        }
        const int off[2] = {0, (int)m};
        if (msorb_pose_optimization_batch(device, 1, &p, off, xy.data(), ur.data(), inv.data(), pos.data(), out.data(), &r, nullptr) != MSORB_OK)
            fail_call("msorb_pose_optimization_batch");
        for (size_t k = 0; k < m; k++) pFrame->mvbOutlier[index[k]] = out[k] != 0;
    }
    pFrame->SetPose(SE3T(QuatT(r.q[3], r.q[0], r.q[1], r.q[2]), VecT(r.t[0], r.t[1], r.t[2])));   // :1033-1035
    return r.n_initial - r.n_bad;   // :1036
}

template <class FrameT>
int PoseOptimization(FrameT* pFrame) {
    return PoseOptimization(pFrame, static_cast<msorb_frame*>(nullptr));
}

// ---------------------------------------------------------------------------------------------------------------------------
// What LocalBundleAdjustment and BundleAdjustment below share.
//
// *flag is a bool another thread may set; the C ABI reads an int, so a watcher thread mirrors the one into the other for as long
// as this object lives (the duration of the call).
class StopFlagMirror {
public:
    explicit StopFlagMirror(bool* flag) : flag_(flag), stop_(flag && *flag ? 1 : 0) {
        if (flag_ && !stop_)
            watcher_ = std::thread([this] {
                while (!done_.load(std::memory_order_acquire)) {
                    if (*static_cast<volatile bool*>(flag_)) { stop_ = 1; return; }
                    std::this_thread::sleep_for(std::chrono::microseconds(50));
                }
            });
    }
    ~StopFlagMirror() {
        done_.store(true, std::memory_order_release);
        if (watcher_.joinable()) watcher_.join();
    }
    const volatile int* get() const { return flag_ ? &stop_ : nullptr; }   // what msorb_local_ba / msorb_bundle_adjustment take

private:
    bool* flag_;
    volatile int stop_;
    std::atomic<bool> done_{false};
    std::thread watcher_;
};

template <class KFPtr>
msorb_ba_keyframe BaKeyFrame(const KFPtr& k, bool fixed) {
    const auto Tcw = k->GetPose();                                                                       // :1133, :1149 / :138
    const auto& q = Tcw.unit_quaternion();
    const auto& t = Tcw.translation();
    msorb_ba_keyframe r;
    r.q[0] = q.x(); r.q[1] = q.y(); r.q[2] = q.z(); r.q[3] = q.w();
    r.t[0] = t(0); r.t[1] = t(1); r.t[2] = t(2);
    r.fx = k->fx; r.fy = k->fy; r.cx = k->cx; r.cy = k->cy; r.mbf = k->mbf;                              // :1267-1271 / :212-216
    r.fixed = fixed ? 1 : 0;
    return r;
}

// the edge arrays of msorb_local_ba / msorb_bundle_adjustment
struct BaEdges {
    std::vector<float> xy, u_right, inv_sigma2;
    std::vector<int> edge_kf, edge_point;
    // the observation of point `point` at keypoint leftIndex of pKF (vertex `kf`); false: the reference makes no edge of it
    template <class KFPtr>
    bool append(const KFPtr& pKF, int leftIndex, int kf, int point) {
        if (leftIndex == -1) return false;
        const float kp_ur = pKF->GetuRight(leftIndex);
        const auto& kpUn = pKF->GetKeyUn(leftIndex);
        if (kpUn.octave > 10) return false;                                                              // :1220, :1249 / :160, :190
        edge_kf.push_back(kf);
        edge_point.push_back(point);
        xy.push_back(kpUn.pt.x); xy.push_back(kpUn.pt.y);
        u_right.push_back(kp_ur < 0 ? -1.0f : kp_ur);                                                    // :1218, :1246 / :158, :187
        inv_sigma2.push_back(pKF->mvInvLevelSigma2[kpUn.octave]);
        return true;
    }
};

// Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1040-1407) on msorb_local_ba.
//
//   bool ORB_SLAM3::msorb_host::LocalBundleAdjustment(pKF, pbStopFlag, pMap, num_fixedKF, num_OptKF, num_MPs, num_edges)
//
// the reference's signature (pKF is its shared_ptr<KeyFrame>), and its effects: the outlier observations erased, SetPose,
// SetWorldPos, UpdateNormalAndDepth, mnOptimizedTimesInLBA++, IncreaseChangeIndex, all under mMutexMapUpdate; num_fixedKF,
// num_OptKF and num_edges as the reference leaves them (it never writes num_MPs, nor does this).  true = done, including the
// reference's two early returns (no fixed KeyFrame, :1098-1102; the stop flag already set, :1323-1325).
//
// false = NOT handled, the map as it was, the caller runs Optimizer::LocalBundleAdjustment: an inertial map (:1113), a KeyFrame
// with a second camera anywhere in the problem (the EdgeSE3ProjectXYZToBody arm, :1281-1317), more free KeyFrames than
// msorb_local_ba_capacity().  The marks mnBALocalForKF / mnBAFixedForKF that the walk sets are put back before a late `false`, so
// the reference's own walk finds them as it would have.
//
// What runs where.  The covisibility walk and the gathering (:1042-1102, :1196-1320) stay host code, as the reference's.  The
// optimisation and the classification (:1326-1373) are the device's.  *pbStopFlag is a bool another thread may set (LocalMapping::
// InterruptBA): StopFlagMirror.
template <class KFPtr, class MPPtr>
struct LocalBAProblem : BaEdges {
    std::list<KFPtr> lLocalKeyFrames, lFixedCameras;
    std::list<MPPtr> lLocalMapPoints;
    std::vector<KFPtr> kf_of_index;        // local KeyFrames first, then the fixed cameras
    std::vector<msorb_ba_keyframe> kfs;
    std::vector<float> pos_w;
    std::vector<std::pair<KFPtr, MPPtr>> edge_objects;
    int num_fixedKF = 0;
    bool two_cameras = false;
    std::vector<std::pair<KFPtr, std::pair<unsigned long, unsigned long>>> kf_marks;   // what the walk overwrote
    std::vector<std::pair<MPPtr, unsigned long>> mp_marks;
    void restore_marks() {
        for (auto it = kf_marks.rbegin(); it != kf_marks.rend(); ++it) { it->first->mnBALocalForKF = it->second.first; it->first->mnBAFixedForKF = it->second.second; }
        for (auto it = mp_marks.rbegin(); it != mp_marks.rend(); ++it) it->first->mnBALocalForKF = it->second;
    }
};

// :1042-1102 and :1196-1320.  Returns the problem as the arrays of msorb_local_ba; kfs / edges are empty when num_fixedKF == 0.
template <class KFPtr, class MapT>
auto GatherLocalBA(KFPtr pKF, MapT* pMap) {
    typedef typename std::decay<decltype(pKF->GetMapPointMatches()[0])>::type MPPtr;
    LocalBAProblem<KFPtr, MPPtr> B;
    auto mark = [&](const KFPtr& k) { B.kf_marks.push_back({k, {k->mnBALocalForKF, k->mnBAFixedForKF}}); };
    B.lLocalKeyFrames.push_back(pKF);
    mark(pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    auto* pCurrentMap = pKF->GetMap();
    const auto vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
    for (size_t i = 0; i < vNeighKFs.size(); i++) {
        KFPtr pKFi = vNeighKFs[i];
        mark(pKFi);
        pKFi->mnBALocalForKF = pKF->mnId;
        if (pKFi->mnId == pMap->GetInitKFid()) B.num_fixedKF = 1;                                        // :1053
        if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) B.lLocalKeyFrames.push_back(pKFi);
    }
    for (const KFPtr& pKFi : B.lLocalKeyFrames) {                                                        // :1063-1077
        const auto vpMPs = pKFi->GetMapPointMatches();
        for (const MPPtr& pMP : vpMPs)
            if (pMP && !pMP->isBad() && pMP->GetMap() == pCurrentMap && pMP->mnBALocalForKF != pKF->mnId) {
                B.lLocalMapPoints.push_back(pMP);
                B.mp_marks.push_back({pMP, pMP->mnBALocalForKF});
                pMP->mnBALocalForKF = pKF->mnId;
            }
    }
    for (const MPPtr& pMP : B.lLocalMapPoints) {                                                         // :1081-1094
        const auto observations = pMP->GetObservations();
        for (const auto& ob : observations) {
            KFPtr pKFi = ob.first;
            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                mark(pKFi);
                pKFi->mnBAFixedForKF = pKF->mnId;
                if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) B.lFixedCameras.push_back(pKFi);
            }
        }
    }
    B.num_fixedKF = (int)B.lFixedCameras.size() + B.num_fixedKF;                                         // :1095
    if (B.num_fixedKF == 0) return B;
    std::map<KFPtr, int> index;
    auto add_kf = [&](const KFPtr& k, bool fixed) {
        index[k] = (int)B.kfs.size();
        B.kfs.push_back(BaKeyFrame(k, fixed));
        B.kf_of_index.push_back(k);
        if (k->mpCamera2) B.two_cameras = true;
    };
    for (const KFPtr& k : B.lLocalKeyFrames) add_kf(k, k->mnId == pMap->GetInitKFid());                  // :1136
    for (const KFPtr& k : B.lFixedCameras) add_kf(k, true);                                              // :1152
    int nPoints = 0;
    for (const MPPtr& pMP : B.lLocalMapPoints) {                                                         // :1196-1320
        const auto Xw = pMP->GetWorldPos();
        B.pos_w.push_back(Xw(0)); B.pos_w.push_back(Xw(1)); B.pos_w.push_back(Xw(2));
        const auto observations = pMP->GetObservations();
        for (const auto& ob : observations) {
            KFPtr pKFi = ob.first;
            if (pKFi->isBad() || pKFi->GetMap() != pCurrentMap) continue;                                // :1214
            const auto at = index.find(pKFi);
            if (at == index.end()) continue;   // (a KeyFrame that is in neither list has no vertex; the reference's setVertex would get NULL)
            if (pKFi->mpCamera2) B.two_cameras = true;
            if (B.append(pKFi, std::get<0>(ob.second), at->second, nPoints)) B.edge_objects.push_back({pKFi, pMP});
        }
        nPoints++;
    }
    return B;
}

template <class KFPtr, class MapT>
bool LocalBundleAdjustment(KFPtr pKF, bool* pbStopFlag, MapT* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs, int& num_edges,
                           int device = 0) {
    (void)num_MPs;
    if (pMap->IsInertial() || pKF->mpCamera2) return false;
    auto B = GatherLocalBA(pKF, pMap);
    if (B.two_cameras || (int)B.kfs.size() - B.num_fixedKF > msorb_local_ba_capacity()) {
        B.restore_marks();
        return false;
    }
    num_fixedKF = B.num_fixedKF;
    if (B.num_fixedKF == 0) return true;                                                                 // :1098-1102
    auto* pCurrentMap = pKF->GetMap();
    pCurrentMap->msOptKFs.clear();                                                                       // :1125-1126, :1141, :1157
    pCurrentMap->msFixedKFs.clear();
    for (const KFPtr& k : B.lLocalKeyFrames) pCurrentMap->msOptKFs.insert(k->mnId);
    for (const KFPtr& k : B.lFixedCameras) pCurrentMap->msFixedKFs.insert(k->mnId);
    num_OptKF = (int)B.lLocalKeyFrames.size();                                                           // :1143
    const int K = (int)B.kfs.size(), P = (int)B.lLocalMapPoints.size(), E = (int)B.edge_kf.size();
    num_edges = E;                                                                                       // :1321
    std::vector<float> kf_out(7 * (size_t)K), pos_out(3 * (size_t)P);
    std::vector<uint8_t> outlier((size_t)E);
    msorb_ba_result r;
    int rc;
    {
        StopFlagMirror stop(pbStopFlag);
        rc = msorb_local_ba(device, K, B.kfs.data(), P, B.pos_w.data(), E, B.edge_kf.data(), B.edge_point.data(), B.xy.data(),
                            B.u_right.data(), B.inv_sigma2.data(), 10, stop.get(), kf_out.data(), nullptr, pos_out.data(), nullptr,
                            outlier.data(), &r, nullptr);
    }
    if (rc == MSORB_E_CAPACITY) { B.restore_marks(); return false; }
    if (rc != MSORB_OK) fail_call("msorb_local_ba");
    if (r.status != 0) return true;                                                                      // :1323-1325
    typedef typename std::decay<decltype(pKF->GetPose())>::type SE3T;
    typedef typename std::decay<decltype(pKF->GetPose().unit_quaternion())>::type QuatT;
    typedef typename std::decay<decltype(pKF->GetPose().translation())>::type VecT;
    typedef typename std::decay<decltype(B.lLocalMapPoints.front()->GetWorldPos())>::type PosT;
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                                            // :1376
    for (int pass = 0; pass < 2; pass++)                                                                 // vToErase: the mono edges, then the stereo edges
        for (int e = 0; e < E; e++) {
            if (!outlier[e] || (B.u_right[e] >= 0) != (pass == 1)) continue;
            const auto& o = B.edge_objects[e];
            if (o.second->isBad()) continue;                                                             // :1335, :1363
            o.first->EraseMapPointMatch(o.second);                                                       // :1382-1383
            o.second->EraseObservation(o.first);
        }
    int k = 0;
    for (const KFPtr& pKFi : B.lLocalKeyFrames) {                                                        // :1388-1395
        const float* o = kf_out.data() + 7 * (size_t)k++;
        pKFi->SetPose(SE3T(QuatT(o[3], o[0], o[1], o[2]), VecT(o[4], o[5], o[6])));
    }
    int p = 0;
    for (const auto& pMP : B.lLocalMapPoints) {                                                          // :1397-1405
        const float* o = pos_out.data() + 3 * (size_t)p++;
        pMP->SetWorldPos(PosT(o[0], o[1], o[2]));
        pMP->UpdateNormalAndDepth();
        pMP->mnOptimizedTimesInLBA++;
    }
    pMap->IncreaseChangeIndex();                                                                         // :1406
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Optimizer::BundleAdjustment and GlobalBundleAdjustemnt (src/Optimizer.cc:51-364) on msorb_bundle_adjustment: the global bundle
// adjustment of the monocular initialisation (Tracking.cc:2561) and of loop closing (LoopClosing.cc:2228).
//
//   bool ORB_SLAM3::msorb_host::BundleAdjustment(vpKFs, vpMP, nIterations = 5, pbStopFlag = NULL, nLoopKF = 0, bRobust = true)
//   bool ORB_SLAM3::msorb_host::GlobalBundleAdjustemnt(pMap, nIterations = 5, pbStopFlag = NULL, nLoopKF = 0, bRobust = true)
//
// the reference's parameter lists and defaults, and its effects: with nLoopKF == pMap->GetOriginKF()->mnId SetPose / SetWorldPos /
// UpdateNormalAndDepth, otherwise mTcwGBA / mPosGBA / mnBAGlobalForKF (:284-288, :356-362), for every KeyFrame that is not bad and
// every point that is not bad and has an observation the reference counts (:154, :261-263).  The counting block of :289-340 has
// no effect and is not restated.  true = done.
//
// false = NOT handled, nothing touched, the caller runs Optimizer::BundleAdjustment: a KeyFrame with a second camera (the
// EdgeSE3ProjectXYZToBody arm, :225-257), or more free KeyFrames than msorb_bundle_adjustment_capacity() (or no room on the device
// for their reduced system).
//
// What runs where.  The gathering (:114-267) stays host code, as the reference's; the optimisation is the device's.  *pbStopFlag is
// a bool another thread may set (LoopClosing's mbStopGBA): StopFlagMirror.
template <class KFPtr, class MPPtr>
bool BundleAdjustment(const std::vector<KFPtr>& vpKFs, const std::vector<MPPtr>& vpMP, int nIterations = 5, bool* pbStopFlag = nullptr,
                      const unsigned long nLoopKF = 0, const bool bRobust = true, int device = 0) {
    if (vpKFs.empty()) return false;
    auto* pMap = vpKFs[0]->GetMap();                                                                     // :66
    std::map<unsigned long, int> index;                                                                  // optimizer.vertex(mnId)
    std::vector<msorb_ba_keyframe> kfs;
    std::vector<KFPtr> kf_of_index;
    unsigned long maxKFid = 0;
    int n_free = 0;
    for (const KFPtr& pKF : vpKFs) {                                                                     // :114-126
        if (pKF->isBad()) continue;
        if (pKF->mpCamera2) return false;
        const msorb_ba_keyframe r = BaKeyFrame(pKF, pKF->mnId == pMap->GetInitKFid());                   // :122
        n_free += r.fixed ? 0 : 1;
        index[pKF->mnId] = (int)kfs.size();
        kfs.push_back(r);
        kf_of_index.push_back(pKF);
        if (pKF->mnId > maxKFid) maxKFid = pKF->mnId;
    }
    if (n_free > msorb_bundle_adjustment_capacity()) return false;
    std::vector<float> pos_w;
    BaEdges G;
    std::vector<MPPtr> mp_of_index;
    std::vector<uint8_t> counted;                                                                        // !vbNotIncludedMP
    for (const MPPtr& pMP : vpMP) {                                                                      // :132-267
        if (pMP->isBad()) continue;
        const auto Xw = pMP->GetWorldPos();
        const int nPoint = (int)mp_of_index.size();
        int nEdges = 0;
        const auto observations = pMP->GetObservations();
        for (const auto& ob : observations) {
            const auto& pKF = ob.first;
            if (pKF->isBad() || pKF->mnId > maxKFid) continue;                                           // :150
            const auto at = index.find(pKF->mnId);
            if (at == index.end()) continue;                                                             // :152
            nEdges++;                                                                                    // :154
            G.append(pKF, std::get<0>(ob.second), at->second, nPoint);
        }
        pos_w.push_back(Xw(0)); pos_w.push_back(Xw(1)); pos_w.push_back(Xw(2));
        mp_of_index.push_back(pMP);
        counted.push_back(nEdges ? 1 : 0);                                                               // :261-266
    }
    const int K = (int)kfs.size(), P = (int)mp_of_index.size(), E = (int)G.edge_kf.size();
    std::vector<float> kf_out(7 * (size_t)K), pos_out(3 * (size_t)P);
    std::vector<uint8_t> included((size_t)P);
    msorb_ba_result r;
    int rc;
    {
        StopFlagMirror stop(pbStopFlag);
        rc = msorb_bundle_adjustment(device, K, kfs.data(), P, pos_w.data(), E, G.edge_kf.data(), G.edge_point.data(), G.xy.data(),
                                     G.u_right.data(), G.inv_sigma2.data(), nIterations, bRobust ? 1 : 0, stop.get(), kf_out.data(),
                                     nullptr, pos_out.data(), nullptr, included.data(), &r, nullptr);
    }
    if (rc == MSORB_E_CAPACITY) return false;
    if (rc != MSORB_OK) fail_call("msorb_bundle_adjustment");
    typedef typename std::decay<decltype(vpKFs[0]->GetPose())>::type SE3T;
    typedef typename std::decay<decltype(vpKFs[0]->GetPose().unit_quaternion())>::type QuatT;
    typedef typename std::decay<decltype(vpKFs[0]->GetPose().translation())>::type VecT;
    const bool bApply = nLoopKF == pMap->GetOriginKF()->mnId;
    for (int k = 0; k < K; k++) {                                                                        // :277-342
        const float* o = kf_out.data() + 7 * (size_t)k;
        const SE3T T(QuatT(o[3], o[0], o[1], o[2]), VecT(o[4], o[5], o[6]));
        if (bApply) {
            kf_of_index[k]->SetPose(T);
        } else {
            kf_of_index[k]->mTcwGBA = T;
            kf_of_index[k]->mnBAGlobalForKF = nLoopKF;
        }
    }
    for (int p = 0; p < P; p++) {                                                                        // :345-363
        if (!counted[p]) continue;   // (a counted point whose observations gave no edge keeps its position: pos_out repeats it)
        typedef typename std::decay<decltype(mp_of_index[p]->GetWorldPos())>::type PosT;
        const float* o = pos_out.data() + 3 * (size_t)p;
        if (bApply) {
            mp_of_index[p]->SetWorldPos(PosT(o[0], o[1], o[2]));
            mp_of_index[p]->UpdateNormalAndDepth();
        } else {
            mp_of_index[p]->mPosGBA = PosT(o[0], o[1], o[2]);
            mp_of_index[p]->mnBAGlobalForKF = nLoopKF;
        }
    }
    return true;
}

template <class MapT>
bool GlobalBundleAdjustemnt(MapT* pMap, int nIterations = 5, bool* pbStopFlag = nullptr, const unsigned long nLoopKF = 0,
                            const bool bRobust = true, int device = 0) {
    const auto vpKFs = pMap->GetAllKeyFrames();                                                          // :53-56
    const auto vpMP = pMap->GetAllMapPoints();
    return BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust, device);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Optimizer::OptimizeSim3 (src/Optimizer.cc:1986-2242 and :2244-2429) on msorb_sim3_optimization_batch.
//
//   int ORB_SLAM3::msorb_host::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints)
//   int ORB_SLAM3::msorb_host::OptimizeSim3(pKF1, pKF2, vpMatches1, vpMatches2, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints)
//
// the reference's two parameter lists, and its effects: vpMatches1[idx] (and vpMatches2[idx] in the second form) reset for the
// pairs that either classification drops, g2oS12 written only when the second optimisation was made, mAcumHessian set to zero
// there and nothing more (the reference never fills it), the return value nIn (0 after the early return of :2211-2212 /
// :2397-2398, which leaves g2oS12 and mAcumHessian as they were).
//
// -1 = NOT handled, nothing touched, the caller keeps Optimizer::OptimizeSim3: a camera that is not Pinhole, a KeyFrame with
// mpCamera2, a gathered keypoint with octave > 10 (for which :2110 and :2134 leave a half-added edge in the reference's graph).
//
// What runs where.  The gathering loops (:2039-2170, :2295-2361) stay host code: they read the map points.  Both optimisations
// and both classifications are one device launch.
struct Sim3OptPairs {
    std::vector<float> P1c, P2c, obs1, obs2, w1, w2;
    std::vector<size_t> vnIndexEdge;
    int nCorrespondences = 0;
    bool handled = true;
    void add(size_t i, const float* p1, const float* p2, float u1, float v1, float u2, float v2, float s1, float s2) {
        P1c.insert(P1c.end(), p1, p1 + 3); P2c.insert(P2c.end(), p2, p2 + 3);
        obs1.push_back(u1); obs1.push_back(v1); obs2.push_back(u2); obs2.push_back(v2);
        w1.push_back(s1); w2.push_back(s2);
        vnIndexEdge.push_back(i);
    }
};

template <class KFPtr>
bool Sim3OptPinholePair(const KFPtr& pKF1, const KFPtr& pKF2) {
    if (pKF1->mpCamera2 || pKF2->mpCamera2) return false;
    return pKF1->mpCamera->GetType() == pKF1->mpCamera->CAM_PINHOLE && pKF2->mpCamera->GetType() == pKF2->mpCamera->CAM_PINHOLE;
}

// :2039-2170
template <class KFPtr, class MPPtr>
Sim3OptPairs GatherSim3Pairs(KFPtr pKF1, KFPtr pKF2, const std::vector<MPPtr>& vpMatches1, const bool bAllPoints) {
    Sim3OptPairs G;
    if (!Sim3OptPinholePair(pKF1, pKF2)) { G.handled = false; return G; }
    const auto R1w = pKF1->GetRotation();
    const auto t1w = pKF1->GetTranslation();
    const auto R2w = pKF2->GetRotation();
    const auto t2w = pKF2->GetTranslation();
    const int N = vpMatches1.size();
    const std::vector<MPPtr> vpMapPoints1 = pKF1->GetMapPointMatches();
    for (int i = 0; i < N; i++) {
        if (!vpMatches1[i]) continue;                                                                    // :2040
        MPPtr pMP1 = vpMapPoints1[i];
        MPPtr pMP2 = vpMatches1[i];
        const int i2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKF2));                                      // :2049
        if (!(pMP1 && pMP2)) continue;                        // :2075-2091: at most a fixed vertex that no edge uses
        if (pMP1->isBad() || pMP2->isBad()) continue;                                                    // :2055, :2071-2074
        const auto P3D1w = pMP1->GetWorldPos();
        const auto P3D1c = (R1w * P3D1w + t1w).eval();                                                           // :2058
        const auto P3D2w = pMP2->GetWorldPos();
        const auto P3D2c = (R2w * P3D2w + t2w).eval();                                                           // :2066
        if (i2 < 0 && !bAllPoints) continue;                                                             // :2093
        if (P3D2c(2) < 0) continue;                                                                      // :2100
        G.nCorrespondences++;                                                                            // :2105
        const auto kpUn1 = pKF1->GetKeyUn(i);
        if (kpUn1.octave > 10) { G.handled = false; return G; }                                          // :2110
        const float invSigmaSquare1 = pKF1->mvInvLevelSigma2[kpUn1.octave];                              // :2120
        float x2, y2;
        int octave2;
        if (i2 >= 0) {                                                                                   // :2132-2139
            const auto kpUn2 = pKF2->GetKeyUn(i2);
            if (kpUn2.octave > 10) { G.handled = false; return G; }
            x2 = kpUn2.pt.x; y2 = kpUn2.pt.y;
            octave2 = kpUn2.octave;
        } else {                                                                                         // :2140-2150
            float invz = 1 / P3D2c(2);
            x2 = P3D2c(0) * invz;
            y2 = P3D2c(1) * invz;
            octave2 = pMP2->mnTrackScaleLevel;
        }
        const float invSigmaSquare2 = pKF2->mvInvLevelSigma2[octave2];                                   // :2157
        const float p1[3] = {P3D1c(0), P3D1c(1), P3D1c(2)}, p2[3] = {P3D2c(0), P3D2c(1), P3D2c(2)};
        G.add((size_t)i, p1, p2, kpUn1.pt.x, kpUn1.pt.y, x2, y2, invSigmaSquare1, invSigmaSquare2);
    }
    return G;
}

// :2295-2361
template <class KFPtr, class MPPtr>
Sim3OptPairs GatherSim3Pairs(KFPtr pKF1, KFPtr pKF2, const std::vector<MPPtr>& vpMatches1, const std::vector<MPPtr>& vpMatches2) {
    Sim3OptPairs G;
    if (!Sim3OptPinholePair(pKF1, pKF2)) { G.handled = false; return G; }
    const auto R1w = pKF1->GetRotation();
    const auto t1w = pKF1->GetTranslation();
    const auto R2w = pKF2->GetRotation();
    const auto t2w = pKF2->GetTranslation();
    const auto O1w = pKF1->GetCameraCenter();
    const auto O2w = pKF2->GetCameraCenter();
    auto* pCamera1 = pKF1->mpCamera;
    auto* pCamera2 = pKF2->mpCamera;
    const int N = vpMatches1.size();
    for (int i = 0; i < N; i++) {
        MPPtr pMP1 = vpMatches1[i];
        MPPtr pMP2 = vpMatches2[i];
        if (!pMP1 || !pMP2 || pMP1->isBad() || pMP2->isBad()) continue;                                  // :2298
        const auto P3D1w = pMP1->GetWorldPos();
        const auto P3D1c = (R1w * P3D1w + t1w).eval();                                                           // :2306
        const auto P3D2w = pMP2->GetWorldPos();
        const auto P3D2c = (R2w * P3D2w + t2w).eval();                                                           // :2314
        G.nCorrespondences++;
        const auto obs1 = pCamera1->project(P3D1c);                                                      // :2323, in float
        const auto PO1 = P3D1w - O1w;
        const float dist1 = PO1.norm();
        const int nPredictedLevel1 = pMP1->PredictScale(dist1, pKF1);                                    // :2331
        const float invSigmaSquare1 = pKF1->mvInvLevelSigma2[nPredictedLevel1];
        const auto obs2 = pCamera2->project(P3D2c);                                                      // :2341
        const auto PO2 = P3D2w - O2w;
        const float dist2 = PO2.norm();
        const int nPredictedLevel2 = pMP2->PredictScale(dist2, pKF2);                                    // :2349
        const float invSigmaSquare2 = pKF2->mvInvLevelSigma2[nPredictedLevel2];
        const float p1[3] = {P3D1c(0), P3D1c(1), P3D1c(2)}, p2[3] = {P3D2c(0), P3D2c(1), P3D2c(2)};
        G.add((size_t)i, p1, p2, obs1(0), obs1(1), obs2(0), obs2(1), invSigmaSquare1, invSigmaSquare2);
    }
    return G;
}

// :2172-2241 / :2363-2428 on the gathered pairs.  bad_out [G.vnIndexEdge.size()] receives the flags.
template <class KFPtr, class Sim3T, class HessianT>
int RunSim3Optimization(const Sim3OptPairs& G, KFPtr pKF1, KFPtr pKF2, Sim3T& g2oS12, const float th2, const bool bFixScale,
                        HessianT& mAcumHessian, int min_pairs, std::vector<uint8_t>& bad, int device) {
    const int n = (int)G.vnIndexEdge.size();
    bad.assign((size_t)n, 0);
    if (n == 0) return 0;                                     // optimize() on an empty graph, then the early return
    msorb_sim3_opt_problem p{};
    const auto& r = g2oS12.rotation();
    const auto& t = g2oS12.translation();
    p.q[0] = r.x(); p.q[1] = r.y(); p.q[2] = r.z(); p.q[3] = r.w();
    p.t[0] = t[0]; p.t[1] = t[1]; p.t[2] = t[2];
    p.s = g2oS12.scale();
    for (int k = 0; k < 4; k++) { p.cam1[k] = pKF1->mpCamera->getParameter(k); p.cam2[k] = pKF2->mpCamera->getParameter(k); }
    p.th2 = th2;
    p.fix_scale = bFixScale ? 1 : 0;
    p.min_pairs = min_pairs;
    p.its[0] = 5; p.its[1] = 10; p.its[2] = 5;                                                           // :2174, :2205-2209
    p.n = n;
    const int off[2] = {0, n};
    msorb_sim3_opt_result res;
    if (msorb_sim3_optimization_batch(device, 1, &p, off, G.P1c.data(), G.P2c.data(), G.obs1.data(), G.obs2.data(), G.w1.data(),
                                      G.w2.data(), bad.data(), nullptr, &res, nullptr) != MSORB_OK)
        fail_call("msorb_sim3_optimization_batch");
    if (res.status != 0) return 0;                                                                       // :2211-2212, :2397-2398
    mAcumHessian.setZero();                                                                              // :2219, :2405
    typedef typename std::decay<decltype(g2oS12.rotation())>::type QuatT;
    typedef typename std::decay<decltype(g2oS12.translation())>::type VecT;
    g2oS12 = Sim3T(QuatT(res.q[3], res.q[0], res.q[1], res.q[2]), VecT(res.t[0], res.t[1], res.t[2]), res.s);   // :2239, :2426
    return res.n_in;
}

template <class KFPtr, class MPPtr, class Sim3T, class HessianT>
int OptimizeSim3(KFPtr pKF1, KFPtr pKF2, std::vector<MPPtr>& vpMatches1, Sim3T& g2oS12, const float th2, const bool bFixScale,
                 HessianT& mAcumHessian, const bool bAllPoints = false, int device = 0) {
    const Sim3OptPairs G = GatherSim3Pairs(pKF1, pKF2, vpMatches1, bAllPoints);
    if (!G.handled) return -1;
    std::vector<uint8_t> bad;
    const int nIn = RunSim3Optimization(G, pKF1, pKF2, g2oS12, th2, bFixScale, mAcumHessian, 10, bad, device);
    for (size_t k = 0; k < bad.size(); k++)
        if (bad[k]) vpMatches1[G.vnIndexEdge[k]].reset();                                                // :2187, :2231
    return nIn;
}

template <class KFPtr, class MPPtr, class Sim3T, class HessianT>
int OptimizeSim3(KFPtr pKF1, KFPtr pKF2, std::vector<MPPtr>& vpMatches1, std::vector<MPPtr>& vpMatches2, Sim3T& g2oS12, const float th2,
                 const bool bFixScale, HessianT& mAcumHessian, const bool bAllPoints = false, int device = 0) {
    (void)bAllPoints;                                         // the reference's second form does not read it either
    const Sim3OptPairs G = GatherSim3Pairs(pKF1, pKF2, vpMatches1, vpMatches2);
    if (!G.handled) return -1;
    std::vector<uint8_t> bad;
    const int nIn = RunSim3Optimization(G, pKF1, pKF2, g2oS12, th2, bFixScale, mAcumHessian, 5, bad, device);
    for (size_t k = 0; k < bad.size(); k++)
        if (bad[k]) {
            vpMatches1[G.vnIndexEdge[k]].reset();                                                        // :2377-2378, :2417-2418
            vpMatches2[G.vnIndexEdge[k]].reset();
        }
    return nIn;
}

}  // namespace msorb_host
}  // namespace ORB_SLAM3

#endif
