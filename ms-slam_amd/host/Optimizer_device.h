// Optimizer::PoseOptimization (src/Optimizer.cc:759-1037), both LocalBundleAdjustment (the local mapper's and the welding one of a map merge), BundleAdjustment / GlobalBundleAdjustemnt, the two OptimizeSim3 and the loop-closing OptimizeEssentialGraph (further down), each on
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
// Scope: pinhole mono / stereo frames.  A frame with a second camera (pFrame->mpCamera2, the arm :870-931) is NOT handled by
// these two: they return -1 without touching the frame (PoseOptimizationAnyCamera below takes such a frame, and a one-camera
// frame whose camera is not a pinhole, to the device; a caller without it keeps Optimizer::PoseOptimization) (the inertial
// variants, PoseInertialOptimizationLastKeyFrame / LastFrame, have templates of their own at the end of this header).  The camera is read from pFrame->fx, fy, cx, cy, mbf, which for Pinhole are the values pCamera->project
// uses (mvParameters[0..3]).
//
// `resident`: a handle whose keypoint table holds THIS frame's mvKeysUn, mvuRight and octaves (DeviceFrame::Upload /
// ExtractStereoFrame of ORBmatcher_device.h).  The handle is filled from mvKeys by the device front-end, so this form is valid
// when mvKeysUn == mvKeys, i.e. for rectified input (Frame::UndistortKeyPoints with mDistCoef(0) == 0, Frame.cc:679-685).  Then
// only the indices of the matched keypoints and their points' positions go up.  Without it everything goes up as flat arrays.
#ifndef MSORB_OPTIMIZER_DEVICE_H
#define MSORB_OPTIMIZER_DEVICE_H

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <thread>
#include <tuple>
#include <utility>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "msorb.h"
#include "../csrc/sim3_opt_device.h"   // the product, inverse and map of Sim3 in double (OptimizeEssentialGraph)
#include "../csrc/inertial_device.h"   // info_from_covariance (InertialOptimization)
#include "../csrc/inertial_plan.h"     // make_plan: the chains the device solves

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

// Optimizer::PoseOptimization for every camera the device knows (msorb_pose_optimization_rig_batch):
//
//   int ORB_SLAM3::msorb_host::PoseOptimizationAnyCamera(Frame* pFrame[, msorb_frame* resident])
//
//   * a pinhole frame without a second camera is handed to PoseOptimization above, `resident` included, and is what that returns;
//   * a frame with a second camera (the arm :870-931, e.g. a KannalaBrandt8 stereo rig): the observation of entry i is mvKeys[i] seen
//     by mpCamera for i < Nleft and mvKeysRight[i - Nleft] seen by mpCamera2 through GetRelativePoseTrl() otherwise;
//   * a one-camera frame whose camera is not a pinhole: mvKeysUn[i] through pCamera->project, as the reference's mono edge has it
//     (PoseOptimization above must NOT be given such a frame: it reads pFrame->fx ... cy and would optimise it as a pinhole).
// The cameras are read through GetType() / getParameter(k) (4 parameters for CAM_PINHOLE, 8 for CAM_FISHEYE).  Effects as the
// reference's: mvbOutlier of every entry with a usable map point, SetPose with the narrowed estimate, the return value
// nInitialCorrespondences - nBad (0, and no SetPose, below three correspondences).  `resident` is not used for these two kinds of
// frame: a handle's keypoint table holds one camera's keys.
// Returns -1 with NOTHING touched, and the caller keeps Optimizer::PoseOptimization, for a camera type other than those two and
// for a one-camera non-pinhole frame with a stereo observation (mvuRight[i] >= 0 on a usable entry: the reference would build a
// pinhole stereo edge from pFrame->fx ... mbf there; the two-camera arm never reads mvuRight).
template <class FrameT>
int PoseOptimizationAnyCamera(FrameT* pFrame, msorb_frame* resident, int device = 0) {
    typedef typename std::decay<decltype(*pFrame->mpCamera)>::type CameraT;
    typedef typename std::decay<decltype(*pFrame->mvpMapPoints[0])>::type MapPointT;
    const bool rig = static_cast<bool>(pFrame->mpCamera2);
    if (!rig && pFrame->mpCamera->GetType() == CameraT::CAM_PINHOLE) return PoseOptimization(pFrame, resident, device);
    msorb_pose_rig_problem p;
    std::memset(&p, 0, sizeof p);
    p.n_cameras = rig ? 2 : 1;
    for (int c = 0; c < p.n_cameras; c++) {
        auto& cam = c == 0 ? *pFrame->mpCamera : *pFrame->mpCamera2;   // (GetType and getParameter are not const in the reference)
        const auto type = cam.GetType();
        int n_par;
        if (type == CameraT::CAM_PINHOLE) { p.cam[c].type = 0; n_par = 4; }
        else if (type == CameraT::CAM_FISHEYE) { p.cam[c].type = 1; n_par = 8; }
        else return -1;
        for (int k = 0; k < n_par; k++) p.cam[c].p[k] = cam.getParameter(k);
    }
    const int N = pFrame->N;
    static thread_local std::vector<uint8_t> camera, out;
    static thread_local std::vector<float> pos, xy, inv;
    static thread_local std::vector<int> index;
    index.clear(); camera.clear(); pos.clear(); xy.clear(); inv.clear();
    {
        std::unique_lock<std::mutex> lock(MapPointT::mGlobalMutex);   // :800
        for (int i = 0; i < N; i++) {
            const auto pMP = pFrame->mvpMapPoints[i];
            if (!(pMP && !pMP->isBad())) continue;                    // :804
            if (!rig && pFrame->mvuRight[i] >= 0) return -1;          // :834: a stereo edge (nothing has been touched yet)
            const bool right = rig && i >= pFrame->Nleft;             // :875, :901
            const auto& kp = !rig ? pFrame->mvKeysUn[i] : right ? pFrame->mvKeysRight[i - pFrame->Nleft] : pFrame->mvKeys[i];   // :813, :876, :902
            xy.push_back(kp.pt.x); xy.push_back(kp.pt.y);
            inv.push_back(pFrame->mvInvLevelSigma2[kp.octave]);       // :820, :887, :913
            camera.push_back(right ? 1 : 0);
            const auto Xw = pMP->GetWorldPos();                       // :828, :895, :921
            pos.push_back(Xw(0)); pos.push_back(Xw(1)); pos.push_back(Xw(2));
            index.push_back(i);
        }
    }
    for (int i : index) pFrame->mvbOutlier[i] = false;                // :810, :878, :907
    const int nInitialCorrespondences = (int)index.size();            // :809, :871
    if (nInitialCorrespondences < 3) return 0;                        // :936-937
    const auto Tcw = pFrame->GetPose();                               // :774
    typedef typename std::decay<decltype(Tcw)>::type SE3T;
    typedef typename std::decay<decltype(Tcw.unit_quaternion())>::type QuatT;
    typedef typename std::decay<decltype(Tcw.translation())>::type VecT;
    {
        const auto& q = Tcw.unit_quaternion();
        const auto& t = Tcw.translation();
        p.q[0] = q.x(); p.q[1] = q.y(); p.q[2] = q.z(); p.q[3] = q.w();
        p.t[0] = t(0); p.t[1] = t(1); p.t[2] = t(2);
    }
    if (rig) {                                                        // :923-924
        const auto Trl = pFrame->GetRelativePoseTrl();
        const auto& q = Trl.unit_quaternion();
        const auto& t = Trl.translation();
        p.q_rl[0] = q.x(); p.q_rl[1] = q.y(); p.q_rl[2] = q.z(); p.q_rl[3] = q.w();
        p.t_rl[0] = t(0); p.t_rl[1] = t(1); p.t_rl[2] = t(2);
    }
    p.n = nInitialCorrespondences;
    msorb_pose_result r;
    out.assign(index.size(), 0);
    const int off[2] = {0, p.n};
    if (msorb_pose_optimization_rig_batch(device, 1, &p, off, xy.data(), camera.data(), inv.data(), pos.data(), out.data(), &r, nullptr) != MSORB_OK)
        fail_call("msorb_pose_optimization_rig_batch");
    for (size_t k = 0; k < index.size(); k++) pFrame->mvbOutlier[index[k]] = out[k] != 0;
    pFrame->SetPose(SE3T(QuatT(r.q[3], r.q[0], r.q[1], r.q[2]), VecT(r.t[0], r.t[1], r.t[2])));   // :1033-1035
    return r.n_initial - r.n_bad;   // :1036
}

template <class FrameT>
int PoseOptimizationAnyCamera(FrameT* pFrame) {
    return PoseOptimizationAnyCamera(pFrame, static_cast<msorb_frame*>(nullptr));
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
// The second Optimizer::LocalBundleAdjustment (src/Optimizer.cc:3494-3915) on msorb_welding_ba: the welding bundle adjustment
// that LoopClosing::MergeLocal runs when the merged maps are not both inertial (LoopClosing.cc:1571).
//
//   bool ORB_SLAM3::msorb_host::LocalBundleAdjustment(pMainKF, vpAdjustKF, vpFixedKF, pbStopFlag)
//
// the reference's parameter list and its effects: mnBALocalForMerge = pMainKF->mnId on every gathered KeyFrame and point; under
// the map's mMutexMapUpdate the observations of vToErase erased (EraseMapPointMatch + EraseObservation, the mono edges first),
// SetPose for every vpAdjustKF that is not bad, SetWorldPos + UpdateNormalAndDepth for every gathered point that is not bad.
// true = done, including the stop flag found set before optimize (:3709-3711: the marks alone).
//
// false = NOT handled, the marks put back, the caller runs Optimizer::LocalBundleAdjustment: a gathered KeyFrame whose camera is
// not a pinhole, more adjustable KeyFrames than msorb_welding_ba_capacity() (or no room on the device for their reduced system).
//
// What is not restated because it has no effect: the counting loops of :3819-3840 and :3852-3899 and their maps (mpObsKFs,
// mpObsFinalKFs, mpObsMPs); :3883 indexes vpEdgeKFMono with a stereo edge's index, past its end when there are more stereo edges.
// What the reference leaves undefined is skipped: an observation whose KeyFrame carries the mark without being a vertex (the mark
// of an earlier merge with the same pMainKF), and the write-back of a vpAdjustKF that is in another map (it has no vertex, :3848
// would read NULL).  A KeyFrame in both lists keeps the fixed vertex, as g2o's addVertex refuses the second one; its SetPose
// receives the bits of its own pose, where the reference hands back the fixed vertex's estimate, the same pose with the quaternion
// normalised in double and narrowed again (equal up to the last bit of a component).
//
// What runs where.  The gathering (:3515-3707) stays host code, as the reference's; both optimisations and both classifications
// are the device's.  *pbStopFlag is a bool another thread may set (LoopClosing's mbStopGBA): StopFlagMirror.
template <class KFPtr, class MPPtr>
struct WeldingBAProblem : BaEdges {
    std::vector<KFPtr> kf_of_index;        // vpFixedKF first, then vpAdjustKF
    std::vector<msorb_ba_keyframe> kfs;
    std::map<unsigned long, int> index;    // optimizer.vertex(mnId)
    int n_free = 0;
    std::vector<MPPtr> vpMPs;              // :3498, in the order of the walk
    std::vector<int> vertex_of_mp;         // per vpMPs entry: its point index, -1 = bad when the vertices were made (:3616)
    std::vector<float> pos_w;
    std::vector<std::pair<KFPtr, MPPtr>> edge_objects;
    bool pinhole = true;
    std::vector<std::pair<KFPtr, unsigned long>> kf_marks;   // what the walk overwrote
    std::vector<std::pair<MPPtr, unsigned long>> mp_marks;
    void restore_marks() {
        for (auto it = kf_marks.rbegin(); it != kf_marks.rend(); ++it) it->first->mnBALocalForMerge = it->second;
        for (auto it = mp_marks.rbegin(); it != mp_marks.rend(); ++it) it->first->mnBALocalForMerge = it->second;
    }
};

// :3515-3707.  Returns the problem as the arrays of msorb_welding_ba.
template <class KFPtr>
auto GatherWeldingBA(KFPtr pMainKF, const std::vector<KFPtr>& vpAdjustKF, const std::vector<KFPtr>& vpFixedKF) {
    typedef typename std::decay<decltype(*pMainKF->GetMapPoints().begin())>::type MPPtr;
    WeldingBAProblem<KFPtr, MPPtr> B;
    const unsigned long id = pMainKF->mnId;
    auto* pCurrentMap = pMainKF->GetMap();
    unsigned long maxKFid = 0;
    auto add = [&](const KFPtr& pKFi, bool fixed) {                                                      // :3522-3552, :3557-3585
        if (pKFi->isBad() || pKFi->GetMap() != pCurrentMap) return;
        B.kf_marks.push_back({pKFi, pKFi->mnBALocalForMerge});
        pKFi->mnBALocalForMerge = id;
        if (pKFi->mpCamera->GetType() != pKFi->mpCamera->CAM_PINHOLE) B.pinhole = false;
        if (!B.index.count(pKFi->mnId)) {
            B.index[pKFi->mnId] = (int)B.kfs.size();
            B.kfs.push_back(BaKeyFrame(pKFi, fixed));
            B.kf_of_index.push_back(pKFi);
            B.n_free += fixed ? 0 : 1;
        }
        if (pKFi->mnId > maxKFid) maxKFid = pKFi->mnId;
        const auto spViewMPs = pKFi->GetMapPoints();
        for (const MPPtr& pMPi : spViewMPs)
            if (pMPi && !pMPi->isBad() && pMPi->GetMap() == pCurrentMap && pMPi->mnBALocalForMerge != id) {
                B.vpMPs.push_back(pMPi);
                B.mp_marks.push_back({pMPi, pMPi->mnBALocalForMerge});
                pMPi->mnBALocalForMerge = id;
            }
    };
    for (const KFPtr& pKFi : vpFixedKF) add(pKFi, true);
    for (const KFPtr& pKFi : vpAdjustKF) add(pKFi, false);
    int nPoints = 0;
    for (const MPPtr& pMPi : B.vpMPs) {                                                                  // :3614-3707
        if (pMPi->isBad()) { B.vertex_of_mp.push_back(-1); continue; }
        B.vertex_of_mp.push_back(nPoints);
        const auto Xw = pMPi->GetWorldPos();
        B.pos_w.push_back(Xw(0)); B.pos_w.push_back(Xw(1)); B.pos_w.push_back(Xw(2));
        const auto observations = pMPi->GetObservations();
        for (const auto& ob : observations) {
            const KFPtr& pKF = ob.first;
            const int leftIndex = std::get<0>(ob.second);
            if (pKF->isBad() || pKF->mnId > maxKFid || pKF->mnBALocalForMerge != id || leftIndex < 0 || !pKF->GetMapPoint(leftIndex)) continue;   // :3633-3635
            const auto at = B.index.find(pKF->mnId);
            if (at == B.index.end()) continue;
            if (B.append(pKF, leftIndex, at->second, nPoints)) B.edge_objects.push_back({pKF, pMPi});    // :3638: octave > 10 makes no edge
        }
        nPoints++;
    }
    return B;
}

template <class KFPtr>
bool LocalBundleAdjustment(KFPtr pMainKF, std::vector<KFPtr> vpAdjustKF, std::vector<KFPtr> vpFixedKF, bool* pbStopFlag, int device = 0) {
    auto B = GatherWeldingBA(pMainKF, vpAdjustKF, vpFixedKF);
    if (!B.pinhole || B.n_free > msorb_welding_ba_capacity()) {
        B.restore_marks();
        return false;
    }
    const int K = (int)B.kfs.size(), P = (int)B.pos_w.size() / 3, E = (int)B.edge_kf.size();
    std::vector<float> kf_out(7 * (size_t)K), pos_out(3 * (size_t)P);
    std::vector<uint8_t> level1((size_t)E), outlier((size_t)E);
    msorb_welding_ba_result r;
    int rc;
    {
        StopFlagMirror stop(pbStopFlag);
        rc = msorb_welding_ba(device, K, B.kfs.data(), P, B.pos_w.data(), E, B.edge_kf.data(), B.edge_point.data(), B.xy.data(),
                              B.u_right.data(), B.inv_sigma2.data(), stop.get(), kf_out.data(), nullptr, pos_out.data(), nullptr,
                              level1.data(), outlier.data(), &r, nullptr);
    }
    if (rc == MSORB_E_CAPACITY) { B.restore_marks(); return false; }
    if (rc != MSORB_OK) fail_call("msorb_welding_ba");
    if (r.status == 2) return true;                                                                      // :3709-3711
    typedef typename std::decay<decltype(pMainKF->GetPose())>::type SE3T;
    typedef typename std::decay<decltype(pMainKF->GetPose().unit_quaternion())>::type QuatT;
    typedef typename std::decay<decltype(pMainKF->GetPose().translation())>::type VecT;
    std::unique_lock<std::mutex> lock(pMainKF->GetMap()->mMutexMapUpdate);                               // :3809
    for (int pass = 0; pass < 2; pass++)                                                                 // vToErase: the mono edges, then the stereo edges
        for (int e = 0; e < E; e++) {
            if (!outlier[e] || (B.u_right[e] >= 0) != (pass == 1)) continue;
            const auto& o = B.edge_objects[e];
            if (o.second->isBad()) continue;                                                             // :3773, :3791
            o.first->EraseMapPointMatch(o.second);                                                       // :3815-3816
            o.second->EraseObservation(o.first);
        }
    for (const KFPtr& pKFi : vpAdjustKF) {                                                               // :3844-3902
        if (pKFi->isBad()) continue;
        const auto at = B.index.find(pKFi->mnId);
        if (at == B.index.end() || B.kf_of_index[at->second] != pKFi) continue;
        const float* o = kf_out.data() + 7 * (size_t)at->second;
        pKFi->SetPose(SE3T(QuatT(o[3], o[0], o[1], o[2]), VecT(o[4], o[5], o[6])));
    }
    for (size_t i = 0; i < B.vpMPs.size(); i++) {                                                        // :3905-3914
        const auto& pMPi = B.vpMPs[i];
        if (pMPi->isBad() || B.vertex_of_mp[i] < 0) continue;
        typedef typename std::decay<decltype(pMPi->GetWorldPos())>::type PosT;
        const float* o = pos_out.data() + 3 * (size_t)B.vertex_of_mp[i];
        pMPi->SetWorldPos(PosT(o[0], o[1], o[2]));
        pMPi->UpdateNormalAndDepth();
    }
    return true;
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

// ---------------------------------------------------------------------------------------------------------------------------
// Optimizer::OptimizeEssentialGraph, the loop-closing overload (src/Optimizer.cc:1410-1675, LoopClosing.cc:1137), on
// msorb_essential_graph.  The merge overload (:1677-1985) follows it.
//
//   bool ORB_SLAM3::msorb_host::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections,
//                                                      bFixScale)
//
// the reference's parameter list, and its effects: under pMap->mMutexMapUpdate SetPose of every KeyFrame with the corrected Sim3 as
// [R t / s], every point that is not bad moved by correctedSwr.map(Srw.map(P)) through its reference KeyFrame (mnCorrectedReference
// when mnCorrectedByKF == pCurKF->mnId) and UpdateNormalAndDepth, then IncreaseChangeIndex.  true = done.
//
// false = NOT handled, nothing touched, the caller runs Optimizer::OptimizeEssentialGraph: a KeyFrame of GetAllKeyFrames() that is
// bad (the reference would dereference its missing vertex at :1639-1640), a KeyFrame id above GetMaxKFid() (the reference would read
// past its vectors), or more free KeyFrames than msorb_essential_graph_capacity() (or no room on the device for their system).
// An edge to a KeyFrame that is no vertex (a parent, loop edge or mPrevKF outside GetAllKeyFrames()) is not added, as g2o's addEdge
// refuses it, and the rest is optimised.
//
// What runs where.  The vertex loop, the CorrectedSim3 / NonCorrectedSim3 look-ups, the weight gate, the five edge arms and the
// measurements Sjw * Swi (double, through the product and inverse of csrc/sim3_opt_device.h: the device's own) stay host code, as
// the reference's; optimize(20) is the device's.  Sophus' cast<double>() of a pose normalises the widened quaternion again
// (so3.hpp:401-408): restated as q / sqrt(((x^2 + y^2) + z^2) + w^2).
template <class S>
inline msorb::sim3opt::Sim3 EgSim3(const S& s) {
    const auto q = s.rotation();
    const auto t = s.translation();
    return msorb::sim3opt::Sim3{(double)q.x(), (double)q.y(), (double)q.z(), (double)q.w(), (double)t(0), (double)t(1), (double)t(2),
                                (double)s.scale()};
}

template <class MapT, class KFPtr, class PoseMapT, class ConnectionsT>
bool OptimizeEssentialGraph(MapT* pMap, KFPtr pLoopKF, KFPtr pCurKF, const PoseMapT& NonCorrectedSim3, const PoseMapT& CorrectedSim3,
                            const ConnectionsT& LoopConnections, const bool& bFixScale, int device = 0) {
    using msorb::sim3opt::Sim3;
    using msorb::sim3opt::sim3_inverse;
    using msorb::sim3opt::sim3_mul;
    const auto vpKFs = pMap->GetAllKeyFrames();                                                          // :1426-1427
    const auto vpMPs = pMap->GetAllMapPoints();
    const unsigned long nMaxKFid = pMap->GetMaxKFid();
    const Sim3 identity{0, 0, 0, 1, 0, 0, 0, 1};                                                         // g2o::Sim3(): what the vectors of :1431-1432 hold by default
    std::vector<Sim3> vScw(nMaxKFid + 1, identity);
    std::vector<int> index(nMaxKFid + 1, -1);                                                            // optimizer.vertex(mnId)
    std::vector<msorb_eg_vertex> vertices;
    const int minFeat = 100;                                                                             // :1439
    int n_free = 0;
    for (const auto& pKF : vpKFs) {                                                                      // :1442-1473
        if (pKF->isBad()) return false;
        const unsigned long nIDi = pKF->mnId;
        const auto it = CorrectedSim3.find(pKF);
        if (it != CorrectedSim3.end()) {
            vScw[nIDi] = EgSim3(it->second);
        } else {                                                                                         // :1456-1457
            const auto Tcw = pKF->GetPose();
            const auto q = Tcw.unit_quaternion();
            const auto t = Tcw.translation();
            const double x = (double)q.x(), y = (double)q.y(), z = (double)q.z(), w = (double)q.w();
            const double len = std::sqrt(((x * x + y * y) + z * z) + w * w);
            vScw[nIDi] = Sim3{x / len, y / len, z / len, w / len, (double)t(0), (double)t(1), (double)t(2), 1.0};
        }
        msorb_eg_vertex v;
        const Sim3& S = vScw[nIDi];
        v.q[0] = S.qx; v.q[1] = S.qy; v.q[2] = S.qz; v.q[3] = S.qw; v.t[0] = S.tx; v.t[1] = S.ty; v.t[2] = S.tz; v.s = S.s;
        v.fixed = pKF->mnId == pMap->GetInitKFid() ? 1 : 0;                                              // :1462-1463
        v.fix_scale = bFixScale ? 1 : 0;                                                                 // :1467
        n_free += v.fixed ? 0 : 1;
        index[nIDi] = (int)vertices.size();
        vertices.push_back(v);
    }
    if (n_free > msorb_essential_graph_capacity()) return false;
    std::vector<int> v0, v1;
    std::vector<double> meas;
    bool missing = false;
    auto add_edge = [&](unsigned long nIDi, unsigned long nIDj, const Sim3& Sji) {   // vertex 0 = i, vertex 1 = j
        if (nIDi > nMaxKFid || nIDj > nMaxKFid) { missing = true; return; }   // (the reference would read past its vectors)
        if (index[nIDi] < 0 || index[nIDj] < 0) return;   // optimizer.vertex() is null: g2o's addEdge refuses the edge, the rest goes on
        v0.push_back(index[nIDi]);
        v1.push_back(index[nIDj]);
        const double m[8] = {Sji.qx, Sji.qy, Sji.qz, Sji.qw, Sji.tx, Sji.ty, Sji.tz, Sji.s};
        meas.insert(meas.end(), m, m + 8);
    };
    auto non_corrected = [&](const KFPtr& pKFx) -> Sim3 {                            // "if in NonCorrectedSim3, that; else vScw"
        const auto itx = NonCorrectedSim3.find(pKFx);
        if (itx != NonCorrectedSim3.end()) return EgSim3(itx->second);
        if (pKFx->mnId > nMaxKFid) { missing = true; return Sim3{0, 0, 0, 1, 0, 0, 0, 1}; }
        return vScw[pKFx->mnId];
    };
    std::set<std::pair<unsigned long, unsigned long>> sInsertedEdges;
    const float ratio = 0.3;                                                                             // :1481
    for (const auto& mit : LoopConnections) {                                                            // :1483-1511
        const KFPtr& pKF = mit.first;
        const unsigned long nIDi = pKF->mnId;
        if (nIDi > nMaxKFid) return false;
        const Sim3 Swi = sim3_inverse(vScw[nIDi]);
        for (const KFPtr& pKFj : mit.second) {
            const unsigned long nIDj = pKFj->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(pKFj) < minFeat * ratio) continue;   // :1494
            if (nIDj > nMaxKFid) return false;
            add_edge(nIDi, nIDj, sim3_mul(vScw[nIDj], Swi));
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }
    for (const KFPtr& pKF : vpKFs) {                                                                     // :1514-1625
        const unsigned long nIDi = pKF->mnId;
        const Sim3 Swi = sim3_inverse(non_corrected(pKF));                                               // :1521-1526
        const KFPtr pParentKF = pKF->GetParent();
        if (pParentKF) add_edge(nIDi, pParentKF->mnId, sim3_mul(non_corrected(pParentKF), Swi));         // :1531-1551
        const auto sLoopEdges = pKF->GetLoopEdges();                                                     // :1554-1576
        for (const KFPtr& pLKF : sLoopEdges)
            if (pLKF->mnId < pKF->mnId) add_edge(nIDi, pLKF->mnId, sim3_mul(non_corrected(pLKF), Swi));
        const auto vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);                                 // :1579-1606
        for (const KFPtr& pKFn : vpConnectedKFs) {
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    add_edge(nIDi, pKFn->mnId, sim3_mul(non_corrected(pKFn), Swi));
                }
            }
        }
        if (pKF->bImu && pKF->mPrevKF)                                                                   // :1609-1624: a plain EdgeSim3
            add_edge(nIDi, pKF->mPrevKF->mnId, sim3_mul(non_corrected(pKF->mPrevKF), Swi));
    }
    if (missing) return false;
    std::vector<double> est(8 * vertices.size());
    msorb_eg_result r;
    const int rc = msorb_essential_graph(device, (int)vertices.size(), vertices.data(), (int)v0.size(), v0.data(), v1.data(), meas.data(), 20,
                                         est.data(), &r, nullptr);                                      // :1627-1630
    if (rc == MSORB_E_CAPACITY) return false;
    if (rc != MSORB_OK) fail_call("msorb_essential_graph");
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                                            // :1631
    typedef typename std::decay<decltype(vpKFs[0]->GetPose())>::type SE3T;
    typedef typename std::decay<decltype(vpKFs[0]->GetPose().unit_quaternion())>::type QuatT;
    typedef typename std::decay<decltype(vpKFs[0]->GetPose().translation())>::type VecT;
    std::vector<Sim3> vCorrectedSwc(nMaxKFid + 1, identity);
    for (const KFPtr& pKFi : vpKFs) {                                                                    // :1634-1646
        const double* o = est.data() + 8 * (size_t)index[pKFi->mnId];
        const Sim3 CorrectedSiw{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]};
        vCorrectedSwc[pKFi->mnId] = sim3_inverse(CorrectedSiw);
        // translation().cast<float>() / s with the double s: Eigen narrows the scalar to the expression's float first
        // (promote_scalar_arg), so the quotient is float / float
        const float sf = (float)CorrectedSiw.s;
        pKFi->SetPose(SE3T(QuatT((float)o[3], (float)o[0], (float)o[1], (float)o[2]), VecT((float)o[4] / sf, (float)o[5] / sf, (float)o[6] / sf)));
    }
    for (const auto& pMP : vpMPs) {                                                                      // :1649-1671
        if (pMP->isBad()) continue;
        unsigned long nIDr;
        if (pMP->mnCorrectedByKF == pCurKF->mnId) nIDr = pMP->mnCorrectedReference;
        else nIDr = pMP->GetReferenceKeyFrame()->mnId;
        const auto P = pMP->GetWorldPos();
        double x, y, z, cx, cy, cz;
        msorb::sim3opt::sim3_map(vScw[nIDr], (double)P(0), (double)P(1), (double)P(2), x, y, z);         // :1667
        msorb::sim3opt::sim3_map(vCorrectedSwc[nIDr], x, y, z, cx, cy, cz);
        typedef typename std::decay<decltype(pMP->GetWorldPos())>::type PosT;
        pMP->SetWorldPos(PosT((float)cx, (float)cy, (float)cz));
        pMP->UpdateNormalAndDepth();
    }
    pMap->IncreaseChangeIndex();                                                                         // :1674
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Optimizer::OptimizeEssentialGraph, the merge overload (src/Optimizer.cc:1677-1985, LoopClosing.cc:1661), on msorb_essential_graph.
//
//   bool ORB_SLAM3::msorb_host::OptimizeEssentialGraph(pCurKF, vpFixedKFs, vpFixedCorrectedKFs, vpNonFixedKFs, vpNonCorrectedMPs)
//
// the reference's parameter list, and its effects: under pMap->mMutexMapUpdate, for every KeyFrame of vpNonFixedKFs that is not
// bad, mTcwBefMerge = GetPose(), mTwcBefMerge = GetPoseInverse() and SetPose with the corrected Sim3 as [R t / s]; every point of
// vpNonCorrectedMPs that is not bad, with the EraseObservation walk to a reference KeyFrame that is not bad, moved IN FLOAT by
// Twr * TNonCorrectedwr.inverse() * P (the types' own operators, so inside MS-SLAM they are Sophus') and UpdateNormalAndDepth when
// its reference KeyFrame has vpBadPose, left alone otherwise (the "another map" arm, :1980-1982).  true = done.
//
// The three vertex classes (:1713-1805): vpFixedKFs fixed with _fix_scale = true (the only class that sets it, :1731) and
// vpGoodPose; vpFixedCorrectedKFs fixed, vScw from mTcwBefMerge, vpGoodPose and vpBadPose; vpNonFixedKFs free unless already in
// sIdKF, vpBadPose.  The three edge arms (:1816-1929) take the corrected relation when both ends have vpGoodPose, else the
// non-corrected one when both have vpBadPose, else no edge; Swi is the identity unless vpBadPose[i] (:1821-1826), as it stands.
//
// false = NOT handled, nothing touched: a KeyFrame id above GetMaxKFid() (the reference would write past its vectors), a KeyFrame
// that would be added as a vertex twice, or more free KeyFrames than msorb_essential_graph_capacity().
template <class KFPtr, class MPPtr>
bool OptimizeEssentialGraph(KFPtr pCurKF, std::vector<KFPtr>& vpFixedKFs, std::vector<KFPtr>& vpFixedCorrectedKFs,
                            std::vector<KFPtr>& vpNonFixedKFs, std::vector<MPPtr>& vpNonCorrectedMPs, int device = 0) {
    using msorb::sim3opt::Sim3;
    using msorb::sim3opt::sim3_inverse;
    using msorb::sim3opt::sim3_mul;
    auto* pMap = pCurKF->GetMap();                                                                       // :1701-1702
    const unsigned long nMaxKFid = pMap->GetMaxKFid();
    const Sim3 identity{0, 0, 0, 1, 0, 0, 0, 1};                                                         // g2o::Sim3()
    std::vector<Sim3> vScw(nMaxKFid + 1, identity), vCorrectedSwc(nMaxKFid + 1, identity);
    std::vector<char> vpGoodPose(nMaxKFid + 1, 0), vpBadPose(nMaxKFid + 1, 0);
    std::vector<int> index(nMaxKFid + 1, -1);                                                            // optimizer.vertex(mnId)
    std::vector<msorb_eg_vertex> vertices;
    auto sim3_of_pose = [](const auto& Tcw) {   // Tcw.cast<double>() (Sophus normalises the widened quaternion), then Sim3(q, t, 1.0)
        const auto q = Tcw.unit_quaternion();
        const auto t = Tcw.translation();
        const double x = (double)q.x(), y = (double)q.y(), z = (double)q.z(), w = (double)q.w();
        const double len = std::sqrt(((x * x + y * y) + z * z) + w * w);
        return Sim3{x / len, y / len, z / len, w / len, (double)t(0), (double)t(1), (double)t(2), 1.0};
    };
    bool refused = false;
    int n_free = 0;
    auto add_vertex = [&](unsigned long nIDi, const Sim3& S, bool fixed, bool fix_scale) {
        if (index[nIDi] >= 0) { refused = true; return; }
        msorb_eg_vertex v;
        v.q[0] = S.qx; v.q[1] = S.qy; v.q[2] = S.qz; v.q[3] = S.qw; v.t[0] = S.tx; v.t[1] = S.ty; v.t[2] = S.tz; v.s = S.s;
        v.fixed = fixed ? 1 : 0;
        v.fix_scale = fix_scale ? 1 : 0;
        n_free += fixed ? 0 : 1;
        index[nIDi] = (int)vertices.size();
        vertices.push_back(v);
    };
    for (const auto* list : {&vpFixedKFs, &vpFixedCorrectedKFs, &vpNonFixedKFs})
        for (const KFPtr& pKFi : *list)
            if (pKFi->mnId > nMaxKFid) return false;
    for (const KFPtr& pKFi : vpFixedKFs) {                                                               // :1713-1739
        if (pKFi->isBad()) continue;
        const unsigned long nIDi = pKFi->mnId;
        const Sim3 Siw = sim3_of_pose(pKFi->GetPose());
        vCorrectedSwc[nIDi] = sim3_inverse(Siw);
        add_vertex(nIDi, Siw, true, true);
        vpGoodPose[nIDi] = 1;
        vpBadPose[nIDi] = 0;
    }
    std::set<unsigned long> sIdKF;
    for (const KFPtr& pKFi : vpFixedCorrectedKFs) {                                                      // :1743-1773
        if (pKFi->isBad()) continue;
        const unsigned long nIDi = pKFi->mnId;
        const Sim3 Siw = sim3_of_pose(pKFi->GetPose());
        vCorrectedSwc[nIDi] = sim3_inverse(Siw);
        vScw[nIDi] = sim3_of_pose(pKFi->mTcwBefMerge);
        add_vertex(nIDi, Siw, true, false);
        sIdKF.insert(nIDi);
        vpGoodPose[nIDi] = 1;
        vpBadPose[nIDi] = 1;
    }
    for (const KFPtr& pKFi : vpNonFixedKFs) {                                                            // :1775-1805
        if (pKFi->isBad()) continue;
        const unsigned long nIDi = pKFi->mnId;
        if (sIdKF.count(nIDi)) continue;
        const Sim3 Siw = sim3_of_pose(pKFi->GetPose());
        vScw[nIDi] = Siw;
        add_vertex(nIDi, Siw, false, false);
        sIdKF.insert(nIDi);
        vpGoodPose[nIDi] = 0;
        vpBadPose[nIDi] = 1;
    }
    if (refused || n_free > msorb_essential_graph_capacity()) return false;
    std::vector<KFPtr> vpKFs;                                                                            // :1807-1812
    vpKFs.insert(vpKFs.end(), vpFixedKFs.begin(), vpFixedKFs.end());
    vpKFs.insert(vpKFs.end(), vpFixedCorrectedKFs.begin(), vpFixedCorrectedKFs.end());
    vpKFs.insert(vpKFs.end(), vpNonFixedKFs.begin(), vpNonFixedKFs.end());
    const std::set<KFPtr> spKFs(vpKFs.begin(), vpKFs.end());
    std::vector<int> v0, v1;
    std::vector<double> meas;
    const int minFeat = 100;                                                                             // :1711
    for (const KFPtr& pKFi : vpKFs) {                                                                    // :1816-1929
        const unsigned long nIDi = pKFi->mnId;
        Sim3 Swi = identity;
        if (vpBadPose[nIDi]) Swi = sim3_inverse(vScw[nIDi]);                                             // :1825-1826
        // the relation to KeyFrame j, when there is one: corrected for two good poses, else non-corrected for two bad ones
        auto relate = [&](unsigned long nIDj) {
            Sim3 Sjw;
            if (vpGoodPose[nIDi] && vpGoodPose[nIDj]) Sjw = sim3_inverse(vCorrectedSwc[nIDj]);
            else if (vpBadPose[nIDi] && vpBadPose[nIDj]) Sjw = vScw[nIDj];
            else return;
            if (index[nIDi] < 0 || index[nIDj] < 0) return;   // (a flag is only set with a vertex: cannot happen)
            const Sim3 Sji = sim3_mul(Sjw, Swi);
            v0.push_back(index[nIDi]);
            v1.push_back(index[nIDj]);
            const double m[8] = {Sji.qx, Sji.qy, Sji.qz, Sji.qw, Sji.tx, Sji.ty, Sji.tz, Sji.s};
            meas.insert(meas.end(), m, m + 8);
        };
        const KFPtr pParentKFi = pKFi->GetParent();
        if (pParentKFi && spKFs.find(pParentKFi) != spKFs.end()) relate(pParentKFi->mnId);               // :1831-1858
        const auto sLoopEdges = pKFi->GetLoopEdges();                                                    // :1861-1888
        for (const KFPtr& pLKF : sLoopEdges)
            if (spKFs.find(pLKF) != spKFs.end() && pLKF->mnId < pKFi->mnId) relate(pLKF->mnId);
        const auto vpConnectedKFs = pKFi->GetCovisiblesByWeight(minFeat);                                // :1891-1923
        for (const KFPtr& pKFn : vpConnectedKFs)
            if (pKFn && pKFn != pParentKFi && !pKFi->hasChild(pKFn) && !sLoopEdges.count(pKFn) && spKFs.find(pKFn) != spKFs.end())
                if (!pKFn->isBad() && pKFn->mnId < pKFi->mnId) relate(pKFn->mnId);
    }
    std::vector<double> est(8 * vertices.size() + 8);
    msorb_eg_result r;
    const int rc = msorb_essential_graph(device, (int)vertices.size(), vertices.data(), (int)v0.size(), v0.data(), v1.data(), meas.data(), 20,
                                         est.data(), &r, nullptr);                                      // :1932-1933
    if (rc == MSORB_E_CAPACITY) return false;
    if (rc != MSORB_OK) fail_call("msorb_essential_graph");
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                                            // :1935
    for (const KFPtr& pKFi : vpNonFixedKFs) {                                                            // :1938-1953
        if (pKFi->isBad()) continue;
        typedef typename std::decay<decltype(pKFi->GetPose())>::type SE3T;
        typedef typename std::decay<decltype(pKFi->GetPose().unit_quaternion())>::type QuatT;
        typedef typename std::decay<decltype(pKFi->GetPose().translation())>::type VecT;
        const double* o = est.data() + 8 * (size_t)index[pKFi->mnId];
        const double s = o[7];
        // Sophus::SE3d Tiw(rotation, translation / s): the constructor normalises the quaternion, in double; cast<float>() narrows
        // (and SE3T's own constructor normalises again, in float, inside MS-SLAM)
        const double len = std::sqrt(((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) + o[3] * o[3]);
        const SE3T Tiw(QuatT((float)(o[3] / len), (float)(o[0] / len), (float)(o[1] / len), (float)(o[2] / len)),
                       VecT((float)(o[4] / s), (float)(o[5] / s), (float)(o[6] / s)));
        pKFi->mTcwBefMerge = pKFi->GetPose();
        pKFi->mTwcBefMerge = pKFi->GetPoseInverse();
        pKFi->SetPose(Tiw);
    }
    for (const MPPtr& pMPi : vpNonCorrectedMPs) {                                                        // :1956-1983
        if (pMPi->isBad()) continue;
        KFPtr pRefKF = pMPi->GetReferenceKeyFrame();
        while (pRefKF->isBad()) {                                                                        // :1961-1970, as it stands
            if (!pRefKF) break;
            pMPi->EraseObservation(pRefKF);
            pRefKF = pMPi->GetReferenceKeyFrame();
        }
        if (pRefKF->mnId <= nMaxKFid && vpBadPose[pRefKF->mnId]) {
            const auto TNonCorrectedwr = pRefKF->mTwcBefMerge;
            const auto Twr = pRefKF->GetPoseInverse();
            const auto eigCorrectedP3Dw = Twr * TNonCorrectedwr.inverse() * pMPi->GetWorldPos();         // :1976, in float
            pMPi->SetWorldPos(eigCorrectedP3Dw);
            pMPi->UpdateNormalAndDepth();
        }   // else: "MapPoint has a reference KF from another map", nothing done (:1980-1982)
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Optimizer::OptimizeEssentialGraph4DoF (src/Optimizer.cc:5174-5458, LoopClosing.cc:1130-1134: the arm an inertial map with an
// initialised IMU takes) on msorb_essential_graph4.
//
//   bool ORB_SLAM3::msorb_host::OptimizeEssentialGraph4DoF(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections)
//
// the reference's parameter list, and its effects: under pMap->mMutexMapUpdate SetPose of every KeyFrame with the optimised
// Rcw, tcw (through g2o::Sim3(Ri, ti, 1.), i.e. Eigen's matrix-to-quaternion conversion, and Sophus::SE3d, whose constructor
// normalises the quaternion in double, narrowed), every point that is not bad moved by correctedSwr.map(Srw.map(P)) through its
// reference KeyFrame and UpdateNormalAndDepth, then IncreaseChangeIndex.  true = done.
//
// false = NOT handled, nothing touched, the caller runs Optimizer::OptimizeEssentialGraph4DoF: a KeyFrame of GetAllKeyFrames() that
// is bad (the reference would dereference its missing vertex at :5425-5426), a KeyFrame id above GetMaxKFid() (the reference would
// read past its vectors), or more free KeyFrames than msorb_essential_graph4_capacity() (or no room on the device for their
// system).  An edge to a KeyFrame that is no vertex (a loop edge or mPrevKF outside GetAllKeyFrames()) is not added, as g2o's
// addEdge refuses it, and the rest is optimised.
//
// What runs where.  The vertex loop with both ImuCamPose constructors (G2oTypes.cc:25-71 for a KeyFrame outside CorrectedSim3:
// four floats of the KeyFrame widened, the camera pose NOT derived from the body pose; :121-146 from Swc's rotation matrix and
// translation, which drops the Sim3's scale), the look-ups, the weight gate, the edge arms (the spanning-tree arm is dead in this
// fork: pParentKF is NULL at :5297) and the measurements Siw * Sjw^-1 in Sim3 arithmetic, of which the rotation matrix and the
// translation go into the edge, stay host code; optimize(20) is the device's.
inline void EgRotationOfQuaternion(const msorb::sim3opt::Sim3& S, double* R) {   // Eigen's Quaternion::toRotationMatrix, row major
    const double tx = 2 * S.qx, ty = 2 * S.qy, tz = 2 * S.qz;
    const double twx = tx * S.qw, twy = ty * S.qw, twz = tz * S.qw, txx = tx * S.qx, txy = ty * S.qx, txz = tz * S.qx;
    const double tyy = ty * S.qy, tyz = tz * S.qy, tzz = tz * S.qz;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
inline void EgQuaternionOfRotation(const double* m, double* q) {   // Eigen's Quaternion(Matrix3) with its branches -> x, y, z, w
    double t = (m[0] + m[4]) + m[8];
    if (t > 0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(((m[4 * i] - m[4 * j]) - m[4 * k]) + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
}

template <class MapT, class KFPtr, class PoseMapT, class ConnectionsT>
bool OptimizeEssentialGraph4DoF(MapT* pMap, KFPtr pLoopKF, KFPtr pCurKF, const PoseMapT& NonCorrectedSim3, const PoseMapT& CorrectedSim3,
                                const ConnectionsT& LoopConnections, int device = 0) {
    using msorb::sim3opt::Sim3;
    using msorb::sim3opt::sim3_inverse;
    using msorb::sim3opt::sim3_mul;
    const auto vpKFs = pMap->GetAllKeyFrames();                                                          // :5191-5192
    const auto vpMPs = pMap->GetAllMapPoints();
    const unsigned long nMaxKFid = pMap->GetMaxKFid();
    const Sim3 identity{0, 0, 0, 1, 0, 0, 0, 1};                                                         // g2o::Sim3(): what the vectors of :5196-5197 hold by default
    std::vector<Sim3> vScw(nMaxKFid + 1, identity);
    std::vector<int> index(nMaxKFid + 1, -1);                                                            // optimizer.vertex(mnId)
    std::vector<msorb_eg4_vertex> vertices;
    const int minFeat = 100;                                                                             // :5201
    int n_free = 0;
    auto mul3 = [](const double* A, const double* B, double* C) {
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
    };
    for (const auto& pKF : vpKFs) {                                                                      // :5203-5236
        if (pKF->isBad()) return false;
        const unsigned long nIDi = pKF->mnId;
        if (nIDi > nMaxKFid) return false;
        msorb_eg4_vertex v;
        const auto Rcb = pKF->mImuCalib.mTcb.rotationMatrix();                                           // G2oTypes.cc:49-50, :132-133
        const auto tcb = pKF->mImuCalib.mTcb.translation();
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) v.Rcb[3 * r + c] = (double)Rcb(r, c);
            v.tcb[r] = (double)tcb(r);
        }
        const auto it = CorrectedSim3.find(pKF);
        if (it != CorrectedSim3.end()) {                                                                 // :5214-5219
            vScw[nIDi] = EgSim3(it->second);
            const Sim3 Swc = sim3_inverse(vScw[nIDi]);
            double Rwc[9];
            EgRotationOfQuaternion(Swc, Rwc);
            const double twc[3] = {Swc.tx, Swc.ty, Swc.tz};
            for (int r = 0; r < 3; r++)                                                                  // G2oTypes.cc:136: twb = Rwc tcb + twc
                v.twb[r] = ((Rwc[3 * r] * v.tcb[0] + Rwc[3 * r + 1] * v.tcb[1]) + Rwc[3 * r + 2] * v.tcb[2]) + twc[r];
            mul3(Rwc, v.Rcb, v.Rwb);                                                                     // :137
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) v.Rcw[3 * r + c] = Rwc[3 * c + r];                           // :138
            for (int r = 0; r < 3; r++)                                                                  // :139: tcw = -Rcw twc
                v.tcw[r] = -((v.Rcw[3 * r] * twc[0] + v.Rcw[3 * r + 1] * twc[1]) + v.Rcw[3 * r + 2] * twc[2]);
        } else {                                                                                         // :5221-5225
            const auto Tcw = pKF->GetPose();
            const auto q = Tcw.unit_quaternion();
            const auto t = Tcw.translation();
            const double x = (double)q.x(), y = (double)q.y(), z = (double)q.z(), w = (double)q.w();
            const double len = std::sqrt(((x * x + y * y) + z * z) + w * w);
            vScw[nIDi] = Sim3{x / len, y / len, z / len, w / len, (double)t(0), (double)t(1), (double)t(2), 1.0};
            const auto Rwb = pKF->GetImuRotation();                                                      // G2oTypes.cc:28-29, :47-48
            const auto twb = pKF->GetImuPosition();
            const auto Rcw = pKF->GetRotation();
            const auto tcw = pKF->GetTranslation();
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) { v.Rwb[3 * r + c] = (double)Rwb(r, c); v.Rcw[3 * r + c] = (double)Rcw(r, c); }
                v.twb[r] = (double)twb(r);
                v.tcw[r] = (double)tcw(r);
            }
        }
        v.fixed = pKF == pLoopKF ? 1 : 0;                                                                // :5228-5229
        v.reserved = 0;
        n_free += v.fixed ? 0 : 1;
        index[nIDi] = (int)vertices.size();
        vertices.push_back(v);
    }
    if (n_free > msorb_essential_graph4_capacity()) return false;
    std::vector<int> v0, v1;
    std::vector<double> meas;
    bool missing = false;
    auto add_edge = [&](unsigned long nIDi, unsigned long nIDj, const Sim3& Sij) {   // vertex 0 = i, vertex 1 = j
        if (nIDi > nMaxKFid || nIDj > nMaxKFid) { missing = true; return; }   // (the reference would read past its vectors)
        if (index[nIDi] < 0 || index[nIDj] < 0) return;   // optimizer.vertex() is null: g2o's addEdge refuses the edge, the rest goes on
        v0.push_back(index[nIDi]);
        v1.push_back(index[nIDj]);
        double m[12];                                                          // Tij: the rotation matrix and the translation; the scale is dropped
        EgRotationOfQuaternion(Sij, m);
        m[9] = Sij.tx; m[10] = Sij.ty; m[11] = Sij.tz;
        meas.insert(meas.end(), m, m + 12);
    };
    auto inverse_non_corrected = [&](const KFPtr& pKFx) -> Sim3 {              // "if in NonCorrectedSim3, that; else vScw", inverted
        const auto itx = NonCorrectedSim3.find(pKFx);
        if (itx != NonCorrectedSim3.end()) return sim3_inverse(EgSim3(itx->second));
        if (pKFx->mnId > nMaxKFid) { missing = true; return Sim3{0, 0, 0, 1, 0, 0, 0, 1}; }
        return sim3_inverse(vScw[pKFx->mnId]);
    };
    std::set<std::pair<unsigned long, unsigned long>> sInsertedEdges;
    const float ratio = 0.3;                                                                             // :5246
    for (const auto& mit : LoopConnections) {                                                            // :5248-5278
        const KFPtr& pKF = mit.first;
        const unsigned long nIDi = pKF->mnId;
        if (nIDi > nMaxKFid) return false;
        const Sim3 Siw = vScw[nIDi];
        for (const KFPtr& pKFj : mit.second) {
            const unsigned long nIDj = pKFj->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(pKFj) < minFeat * ratio) continue;   // :5258
            if (nIDj > nMaxKFid) return false;
            add_edge(nIDi, nIDj, sim3_mul(Siw, sim3_inverse(vScw[nIDj])));                               // :5261-5262
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }
    for (const KFPtr& pKF : vpKFs) {                                                                     // :5281-5411
        const unsigned long nIDi = pKF->mnId;
        Sim3 Siw;                                                                                        // :5286-5294
        const auto iti = NonCorrectedSim3.find(pKF);
        if (iti != NonCorrectedSim3.end()) Siw = EgSim3(iti->second);
        else Siw = vScw[nIDi];
        const KFPtr pParentKF;                                                                           // :5297: NULL, the spanning-tree arm (:5298-5321) is dead
        const KFPtr prevKF = pKF->mPrevKF;                                                               // :5324-5348
        if (prevKF) add_edge(nIDi, prevKF->mnId, sim3_mul(Siw, inverse_non_corrected(prevKF)));
        const auto sLoopEdges = pKF->GetLoopEdges();                                                     // :5351-5377
        for (const KFPtr& pLKF : sLoopEdges)
            if (pLKF->mnId < pKF->mnId) add_edge(nIDi, pLKF->mnId, sim3_mul(Siw, inverse_non_corrected(pLKF)));
        const auto vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);                                 // :5380-5410
        for (const KFPtr& pKFn : vpConnectedKFs) {
            if (pKFn && pKFn != pParentKF && pKFn != prevKF && pKFn != pKF->mNextKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    add_edge(nIDi, pKFn->mnId, sim3_mul(Siw, inverse_non_corrected(pKFn)));
                }
            }
        }
    }
    if (missing) return false;
    std::vector<double> poses(12 * vertices.size());
    msorb_eg4_result r;
    const int rc = msorb_essential_graph4(device, (int)vertices.size(), vertices.data(), (int)v0.size(), v0.data(), v1.data(), meas.data(),
                                          20, poses.data(), &r, nullptr);                               // :5413-5415
    if (rc == MSORB_E_CAPACITY) return false;
    if (rc != MSORB_OK) fail_call("msorb_essential_graph4");
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                                            // :5417
    typedef typename std::decay<decltype(vpKFs[0]->GetPose())>::type SE3T;
    typedef typename std::decay<decltype(vpKFs[0]->GetPose().unit_quaternion())>::type QuatT;
    typedef typename std::decay<decltype(vpKFs[0]->GetPose().translation())>::type VecT;
    std::vector<Sim3> vCorrectedSwc(nMaxKFid + 1, identity);
    for (const KFPtr& pKFi : vpKFs) {                                                                    // :5420-5434
        const double* o = poses.data() + 12 * (size_t)index[pKFi->mnId];
        double q[4];
        EgQuaternionOfRotation(o, q);                                                                    // g2o::Sim3(Ri, ti, 1.) (:5429)
        const Sim3 CorrectedSiw{q[0], q[1], q[2], q[3], o[9], o[10], o[11], 1.0};
        vCorrectedSwc[pKFi->mnId] = sim3_inverse(CorrectedSiw);
        const double len = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);         // Sophus::SE3d(q, t) normalises (:5432)
        pKFi->SetPose(SE3T(QuatT((float)(q[3] / len), (float)(q[0] / len), (float)(q[1] / len), (float)(q[2] / len)),
                           VecT((float)o[9], (float)o[10], (float)o[11])));
    }
    for (const auto& pMP : vpMPs) {                                                                      // :5437-5456
        if (pMP->isBad()) continue;
        const unsigned long nIDr = pMP->GetReferenceKeyFrame()->mnId;
        const auto P = pMP->GetWorldPos();
        double x, y, z, cx, cy, cz;
        msorb::sim3opt::sim3_map(vScw[nIDr], (double)P(0), (double)P(1), (double)P(2), x, y, z);         // :5452
        msorb::sim3opt::sim3_map(vCorrectedSwc[nIDr], x, y, z, cx, cy, cz);
        typedef typename std::decay<decltype(pMP->GetWorldPos())>::type PosT;
        pMP->SetWorldPos(PosT((float)cx, (float)cy, (float)cz));
        pMP->UpdateNormalAndDepth();
    }
    pMap->IncreaseChangeIndex();                                                                         // :5457
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Optimizer::InertialOptimization (src/Optimizer.cc:3050-3227, :3230-3384, :3386-3491; LocalMapping.cc:1288 InitializeIMU,
// LoopClosing.cc:1807 after a merge, LocalMapping.cc:1481 ScaleRefinement) on msorb_inertial_optimization.
//
//   bool ORB_SLAM3::msorb_host::InertialOptimization(pMap, Rwg, scale, bg, ba, bMono, covInertial, bFixedVel, bGauss, priorG, priorA)
//   bool ORB_SLAM3::msorb_host::InertialOptimization(pMap, bg, ba, priorG, priorA)
//   bool ORB_SLAM3::msorb_host::InertialOptimization(pMap, Rwg, scale)
//
// the reference's parameter lists (a trailing `device` besides), and its effects.  Gathering stays host code, in the reference's
// order: the `mnId > maxKFid` skips, mpImuPreintegrated->SetNewBias(mPrevKF->GetImuBias()) per edge in the first two overloads
// only, the bias vertices built from vpKFs.front() (in the third overload one pair per KeyFrame, all from vpKFs.front() alike).
// Afterwards scale, Rwg, bg, ba are written, every KeyFrame with a vertex gets SetVelocity(Vw.cast<float>()) and SetNewBias(b), with
// Reintegrate() when (GetGyroBias() - bg.cast<float>()).norm() > 0.01 held before the new bias was set (:3218-3223).  The third
// overload writes scale and Rwg only; its two activeRobustChi2 floats have no effect and are not restated.  covInertial and bGauss
// are read by nothing in the reference; bMono only frees the scale (:3131).  bg and ba are outputs: the estimates start from
// vpKFs.front()'s biases.
//
// false = NOT handled, nothing touched (decided before the first side effect), the caller runs Optimizer::InertialOptimization: an
// empty map, more KeyFrames than msorb_inertial_optimization_capacity(), an edge whose KeyFrame lacks mpImuPreintegrated, an edge
// whose mPrevKF has no vertex (not among GetAllKeyFrames(): the reference's error branch, which dereferences null in the third
// overload), a covariance whose inverse does not exist, a structure the plan rejects (two KeyFrames with one mPrevKF).  A device
// error after the gathering also returns false; the SetNewBias calls made until then are the ones the reference repeats.
namespace inertial_detail {
struct Gathered {
    std::vector<msorb_inertial_keyframe> kfs;
    std::vector<msorb_inertial_edge> edges;
    std::vector<int> edge_kf;                                                                            // per edge: the position of its KeyFrame in vpKFs
};

// Everything the device needs from vpKFs, WITHOUT a side effect, and "would it be handled".  vpKFs and maxKFid are fetched once by
// the caller, as the reference fetches them (:3055-3056), and serve the gathering and the write-back alike.
template <class KFVec>
bool Gather(const KFVec& vpKFs, unsigned long maxKFid, Gathered& G) {
    if (vpKFs.empty() || (int)vpKFs.size() > msorb_inertial_optimization_capacity()) return false;      // (vpKFs.front() of :3094)
    G.kfs.assign(vpKFs.size(), msorb_inertial_keyframe());
    G.edges.clear();
    G.edge_kf.clear();
    std::vector<int> index(maxKFid + 1, -1);                                                             // optimizer.vertex(mnId): position in vpKFs
    for (size_t i = 0; i < vpKFs.size(); i++) {                                                          // :3074-3091
        const auto& pKFi = vpKFs[i];
        msorb_inertial_keyframe& k = G.kfs[i];
        const auto Rwb = pKFi->GetImuRotation();                                                         // ImuCamPose(pKF) (G2oTypes.cc:28-29)
        const auto twb = pKFi->GetImuPosition();
        const auto v = pKFi->GetVelocity();                                                              // VertexVelocity(pKF) (:456-459)
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) k.Rwb[3 * r + c] = (double)Rwb(r, c);
            k.twb[r] = (double)twb(r);
            k.v[r] = (double)v(r);
        }
        k.has_velocity_vertex = pKFi->mnId > maxKFid ? 0 : 1;
        k.reserved = 0;
        if (k.has_velocity_vertex) index[pKFi->mnId] = (int)i;
    }
    std::vector<int> prev, cur;
    for (size_t i = 0; i < vpKFs.size(); i++) {                                                          // :3142-3182
        const auto& pKFi = vpKFs[i];
        if (!(pKFi->mPrevKF && pKFi->mnId <= maxKFid)) continue;
        if (pKFi->isBad() || pKFi->mPrevKF->mnId > maxKFid) continue;
        const auto pInt = pKFi->mpImuPreintegrated;
        if (!pInt) return false;                                                                         // :3148-3151 would dereference it
        const int at = index[pKFi->mPrevKF->mnId];
        if (at < 0 || vpKFs[at] != pKFi->mPrevKF) return false;                                          // :3160-3165: no such vertex
        msorb_inertial_edge e;
        e.kf_prev = at;
        e.kf_cur = (int)i;
        const auto &dR = pInt->dR, &JRg = pInt->JRg, &JVg = pInt->JVg, &JVa = pInt->JVa, &JPg = pInt->JPg, &JPa = pInt->JPa;   // Matrix3f
        const auto &dV = pInt->dV, &dP = pInt->dP;                                                       // Vector3f
        const auto& C = pInt->C;                                                                         // Matrix<float, 15, 15>
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) {
                e.dR[3 * r + c] = dR(r, c); e.JRg[3 * r + c] = JRg(r, c); e.JVg[3 * r + c] = JVg(r, c);
                e.JVa[3 * r + c] = JVa(r, c); e.JPg[3 * r + c] = JPg(r, c); e.JPa[3 * r + c] = JPa(r, c);
            }
            e.dV[r] = dV(r);
            e.dP[r] = dP(r);
        }
        const auto& imuBias = pInt->b;
        e.bias[0] = imuBias.bax; e.bias[1] = imuBias.bay; e.bias[2] = imuBias.baz;
        e.bias[3] = imuBias.bwx; e.bias[4] = imuBias.bwy; e.bias[5] = imuBias.bwz;
        e.dT = pInt->dT;
        float C9[81];
        for (int r = 0; r < 9; r++)
            for (int c = 0; c < 9; c++) C9[9 * r + c] = C(r, c);
        if (!msorb::inertial::info_from_covariance(C9, 9, e.info)) return false;                         // G2oTypes.cc:604-612
        prev.push_back(e.kf_prev);
        cur.push_back(e.kf_cur);
        G.edges.push_back(e);
        G.edge_kf.push_back((int)i);
    }
    msorb::inertial::Plan plan;
    return msorb::inertial::make_plan((int)G.kfs.size(), (int)G.edges.size(), prev.data(), cur.data(), plan) == msorb::inertial::kPlanOk;
}

// which: 1, 2, 3 = the overload
template <class KFVec>
bool Run(const KFVec& vpKFs, unsigned long maxKFid, int which, msorb_inertial_problem& P, Gathered& G, std::vector<double>& v,
         msorb_inertial_result& R, int device) {
    if (!Gather(vpKFs, maxKFid, G)) return false;                                                        // nothing touched so far
    if (which != 3)                                                                                      // :3151, :3316, in the edges' order
        for (int at : G.edge_kf) {
            const auto& pKFi = vpKFs[at];
            const auto pInt = pKFi->mpImuPreintegrated;
            pInt->SetNewBias(pKFi->mPrevKF->GetImuBias());
        }
    const auto& pKF = vpKFs.front();
    const auto bg0 = pKF->GetGyroBias();                                                                 // VertexGyroBias(vpKFs.front()) (:3094, :3418)
    const auto ba0 = pKF->GetAccBias();
    for (int k = 0; k < 3; k++) { P.bg[k] = (double)bg0(k); P.ba[k] = (double)ba0(k); }
    v.assign(3 * G.kfs.size(), 0.0);
    return msorb_inertial_optimization(device, &P, (int)G.kfs.size(), G.kfs.data(), (int)G.edges.size(), G.edges.data(), v.data(), nullptr, &R,
                                       nullptr) == MSORB_OK;
}

// :3193-3226 / :3355-3383, over the vector the velocities were gathered from: v[3 i] belongs to vpKFs[i]
template <class KFVec, class Vec3d>
void WriteBack(const KFVec& vpKFs, unsigned long maxKFid, const std::vector<double>& v, const msorb_inertial_result& R, Vec3d& bg, Vec3d& ba) {
    for (int k = 0; k < 3; k++) { bg(k) = R.bg[k]; ba(k) = R.ba[k]; }
    for (size_t i = 0; i < vpKFs.size(); i++) {
        const auto& pKFi = vpKFs[i];
        if (pKFi->mnId > maxKFid) continue;
        typedef typename std::decay<decltype(pKFi->GetVelocity())>::type VelT;
        typedef typename std::decay<decltype(pKFi->GetImuBias())>::type BiasT;
        pKFi->SetVelocity(VelT((float)v[3 * i], (float)v[3 * i + 1], (float)v[3 * i + 2]));              // :3216
        const BiasT b((float)R.ba[0], (float)R.ba[1], (float)R.ba[2], (float)R.bg[0], (float)R.bg[1], (float)R.bg[2]);   // :3204
        const auto gb = pKFi->GetGyroBias();
        const float dx = gb(0) - (float)R.bg[0], dy = gb(1) - (float)R.bg[1], dz = gb(2) - (float)R.bg[2];
        const float norm = std::sqrt((dx * dx + dy * dy) + dz * dz);                                     // :3218, in float
        if (norm > 0.01) {
            pKFi->SetNewBias(b);
            const auto pInt = pKFi->mpImuPreintegrated;
            if (pInt) pInt->Reintegrate();
        } else {
            pKFi->SetNewBias(b);
        }
    }
}
}  // namespace inertial_detail

template <class MapT, class Mat3d, class Vec3d, class MatXd>
bool InertialOptimization(MapT* pMap, Mat3d& Rwg, double& scale, Vec3d& bg, Vec3d& ba, bool bMono, MatXd& covInertial, bool bFixedVel = false,
                          bool bGauss = false, float priorG = 1e2, float priorA = 1e6, int device = 0) {
    (void)covInertial; (void)bGauss;                                                                     // read by nothing in :3050-3227
    msorb_inertial_problem P = msorb_inertial_problem();
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) P.Rwg[3 * r + c] = Rwg(r, c);
    P.scale = scale;
    P.prior_g = (double)priorG;                                                                          // double infoPriorG = priorG (:3120)
    P.prior_a = (double)priorA;
    P.free_velocities = P.free_biases = bFixedVel ? 0 : 1;                                               // :3085-3106
    P.free_gdir = 1;
    P.free_scale = bMono ? 1 : 0;                                                                        // :3131
    P.with_priors = 1;
    P.algorithm = 0;
    P.user_lambda_init = priorG != 0.f ? 1 : 0;                                                          // :3068-3069
    P.iterations = 200;                                                                                  // :3054
    inertial_detail::Gathered G;
    std::vector<double> v;
    msorb_inertial_result R;
    const unsigned long maxKFid = pMap->GetMaxKFid();                                                    // :3055-3056, once
    const auto vpKFs = pMap->GetAllKeyFrames();
    if (!inertial_detail::Run(vpKFs, maxKFid, 1, P, G, v, R, device)) return false;
    scale = R.scale;                                                                                     // :3191
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Rwg(r, c) = R.Rwg[3 * r + c];                                        // :3205
    inertial_detail::WriteBack(vpKFs, maxKFid, v, R, bg, ba);
    return true;
}

template <class MapT, class Vec3d>
bool InertialOptimization(MapT* pMap, Vec3d& bg, Vec3d& ba, float priorG = 1e2, float priorA = 1e6, int device = 0) {
    msorb_inertial_problem P = msorb_inertial_problem();
    P.Rwg[0] = P.Rwg[4] = P.Rwg[8] = 1.0;                                                                // VertexGDir(Identity), fixed (:3293-3295)
    P.scale = 1.0;                                                                                       // VertexScale(1.0), fixed (:3297-3299)
    P.prior_g = (double)priorG;
    P.prior_a = (double)priorA;
    P.free_velocities = P.free_biases = 1;
    P.with_priors = 1;
    P.user_lambda_init = 1;                                                                              // :3245
    P.iterations = 200;                                                                                  // :3232
    inertial_detail::Gathered G;
    std::vector<double> v;
    msorb_inertial_result R;
    const unsigned long maxKFid = pMap->GetMaxKFid();                                                    // :3233-3234, once
    const auto vpKFs = pMap->GetAllKeyFrames();
    if (!inertial_detail::Run(vpKFs, maxKFid, 2, P, G, v, R, device)) return false;
    inertial_detail::WriteBack(vpKFs, maxKFid, v, R, bg, ba);
    return true;
}

template <class MapT, class Mat3d>
bool InertialOptimization(MapT* pMap, Mat3d& Rwg, double& scale, int device = 0) {
    msorb_inertial_problem P = msorb_inertial_problem();
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) P.Rwg[3 * r + c] = Rwg(r, c);
    P.scale = scale;
    P.free_gdir = P.free_scale = 1;                                                                      // :3431, :3435
    P.algorithm = 1;                                                                                     // :3399 Gauss-Newton
    P.huber = 1;                                                                                         // :3473-3475
    P.iterations = 10;                                                                                   // :3387
    inertial_detail::Gathered G;
    std::vector<double> v;
    msorb_inertial_result R;
    const unsigned long maxKFid = pMap->GetMaxKFid();                                                    // :3388-3389, once
    const auto vpKFs = pMap->GetAllKeyFrames();
    if (!inertial_detail::Run(vpKFs, maxKFid, 3, P, G, v, R, device)) return false;
    scale = R.scale;                                                                                     // :3489
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Rwg(r, c) = R.Rwg[3 * r + c];                                        // :3490
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:4422-4779) and PoseInertialOptimizationLastFrame
// (:4781-5172; Tracking.cc:2946-2968) on msorb_pose_inertial_optimization_batch / msorb_frame_pose_inertial_optimization.
//
//   int ORB_SLAM3::msorb_host::PoseInertialOptimizationLastKeyFrame(Frame* pFrame, bool bRecInit = false)
//   int ORB_SLAM3::msorb_host::PoseInertialOptimizationLastFrame(Frame* pFrame, bool bRecInit = false)
//   ... (Frame* pFrame, msorb_frame* resident, bool bRecInit = false)      keypoints already on a handle, rectified input
//
// the reference's parameter lists and effects, in its order: mvbOutlier of every entry with a map point (`if (pMP)` alone, no
// isBad() here), SetImuPoseVelocity with the narrowed estimate, mImuBias, pFrame->mpcpi = new ConstraintPoseImu(...) and, in the
// LastFrame form, delete pFp->mpcpi; pFp->mpcpi = NULL.  The return value is nInitialCorrespondences - nBad.
//
// The gathering loops (:4473-4576, :4832-4934) stay host code; the information matrices are built here (info_from_covariance
// for the 9x9 of EdgeInertial's constructor, a written-out 3x3 inverse in double for the two random-walk blocks of
// pFrame->mpImuPreintegrated->C, which both forms read: :4610, :4971); then one call.
//
// The library returns H_prior, what ConstraintPoseImu's constructor leaves.  The constructor would clip that matrix once more
// (another eigen-decomposition, not the identity in floating point), so the object is constructed and its public member H is then
// assigned the returned matrix: mpcpi->H is H_prior bit for bit.
//
// -1 = NOT handled, nothing touched, the caller keeps the g2o routine: a second camera (mpCamera2), Nleft != -1, a missing
// preintegration or other end, a covariance without inverse and, in the LastFrame form, !pFp->mpcpi (the reference
// dereferences null there).
namespace pose_inertial_detail {
template <class PreT>
bool EdgeOf(const PreT& pInt, msorb_inertial_edge& e) {
    e.kf_prev = 0;
    e.kf_cur = 0;
    const auto &dR = pInt->dR, &JRg = pInt->JRg, &JVg = pInt->JVg, &JVa = pInt->JVa, &JPg = pInt->JPg, &JPa = pInt->JPa;   // Matrix3f
    const auto &dV = pInt->dV, &dP = pInt->dP;                                                           // Vector3f
    const auto& C = pInt->C;                                                                             // Matrix<float, 15, 15>
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) {
            e.dR[3 * r + c] = dR(r, c); e.JRg[3 * r + c] = JRg(r, c); e.JVg[3 * r + c] = JVg(r, c);
            e.JVa[3 * r + c] = JVa(r, c); e.JPg[3 * r + c] = JPg(r, c); e.JPa[3 * r + c] = JPa(r, c);
        }
        e.dV[r] = dV(r);
        e.dP[r] = dP(r);
    }
    const auto& imuBias = pInt->b;
    e.bias[0] = imuBias.bax; e.bias[1] = imuBias.bay; e.bias[2] = imuBias.baz;
    e.bias[3] = imuBias.bwx; e.bias[4] = imuBias.bwy; e.bias[5] = imuBias.bwz;
    e.dT = pInt->dT;
    float C9[81];
    for (int r = 0; r < 9; r++)
        for (int c = 0; c < 9; c++) C9[9 * r + c] = C(r, c);
    return msorb::inertial::info_from_covariance(C9, 9, e.info);                                         // G2oTypes.cc:500-508
}

// C.block<3, 3>(at, at).cast<double>().inverse() (:4610, :4617): the adjugate over the determinant, in double
template <class PreT>
bool RandomWalkInformation(const PreT& pInt, int at, double* info) {
    double m[9];
    const auto& C = pInt->C;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) m[3 * r + c] = (double)C(at + r, at + c);
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = (m[0] * c00 + m[1] * c01) + m[2] * c02;
    if (!(std::fabs(det) > 0) || !std::isfinite(det)) return false;
    const double inv = 1.0 / det;
    info[0] = c00 * inv; info[1] = (m[2] * m[7] - m[1] * m[8]) * inv; info[2] = (m[1] * m[5] - m[2] * m[4]) * inv;
    info[3] = c01 * inv; info[4] = (m[0] * m[8] - m[2] * m[6]) * inv; info[5] = (m[2] * m[3] - m[0] * m[5]) * inv;
    info[6] = c02 * inv; info[7] = (m[1] * m[6] - m[0] * m[7]) * inv; info[8] = (m[0] * m[4] - m[1] * m[3]) * inv;
    return true;
}

template <class RotT, class VecT, class VelT>
void StateOf(const RotT& Rwb, const VecT& twb, const VelT& v, msorb_pose_inertial_state& s) {
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) s.Rwb[3 * r + c] = (double)Rwb(r, c);
        s.twb[r] = (double)twb(r);
        s.v[r] = (double)v(r);
    }
}
template <class BiasT>
void BiasOf(const BiasT& b, msorb_pose_inertial_state& s) {                                              // G2oTypes.cc:471-488
    s.bg[0] = b.bwx; s.bg[1] = b.bwy; s.bg[2] = b.bwz;
    s.ba[0] = b.bax; s.ba[1] = b.bay; s.ba[2] = b.baz;
}

// form 0: the last KeyFrame; form 1: the previous frame
template <class FrameT>
int Run(FrameT* pFrame, int form, msorb_frame* resident, bool bRecInit, int device) {
    if (pFrame->mpCamera2 || pFrame->Nleft != -1) return -1;
    const auto pIntKF = pFrame->mpImuPreintegrated;                                                      // the random-walk blocks, both forms
    if (!pIntKF) return -1;
    static thread_local msorb_pose_inertial_problem p;
    static thread_local msorb_pose_inertial_result r;
    p = msorb_pose_inertial_problem();
    p.form = form;
    p.rec_init = bRecInit ? 1 : 0;
    auto* pFp = pFrame->mpPrevFrame;
    if (form == 0) {
        const auto pKF = pFrame->mpLastKeyFrame;                                                         // :4579-4595
        if (!pKF) return -1;
        StateOf(pKF->GetImuRotation(), pKF->GetImuPosition(), pKF->GetVelocity(), p.other);
        const auto bg = pKF->GetGyroBias();
        const auto ba = pKF->GetAccBias();
        for (int k = 0; k < 3; k++) { p.other.bg[k] = (double)bg(k); p.other.ba[k] = (double)ba(k); }
        if (!EdgeOf(pIntKF, p.pre)) return -1;                                                           // :4597
    } else {
        if (!pFp || !pFp->mpcpi) return -1;                                                              // :4982-4986
        const auto pIntF = pFrame->mpImuPreintegratedFrame;                                              // :4958
        if (!pIntF || !EdgeOf(pIntF, p.pre)) return -1;
        StateOf(pFp->GetImuRotation(), pFp->GetImuPosition(), pFp->GetVelocity(), p.other);              // :4938-4956
        BiasOf(pFp->mImuBias, p.other);
        const auto* c = pFp->mpcpi;                                                                      // G2oTypes.cc:720-729
        StateOf(c->Rwb, c->twb, c->vwb, p.prior);
        for (int k = 0; k < 3; k++) { p.prior.bg[k] = c->bg(k); p.prior.ba[k] = c->ba(k); }
        for (int a = 0; a < 15; a++)
            for (int b = 0; b < 15; b++) p.H[15 * a + b] = c->H(a, b);
    }
    if (!RandomWalkInformation(pIntKF, 9, p.info_gyro) || !RandomWalkInformation(pIntKF, 12, p.info_acc)) return -1;   // :4610, :4617
    StateOf(pFrame->GetImuRotation(), pFrame->GetImuPosition(), pFrame->GetVelocity(), p.frame);         // :4439-4454
    BiasOf(pFrame->mImuBias, p.frame);
    {
        const auto Tcw = pFrame->GetPose();                                                              // G2oTypes.cc:95-100
        const auto Rcw = Tcw.rotationMatrix();
        const auto tcw = Tcw.translation();
        const auto Rcb = pFrame->mImuCalib.mTcb.rotationMatrix();
        const auto tcb = pFrame->mImuCalib.mTcb.translation();
        const auto tbc = pFrame->mImuCalib.mTbc.translation();
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) { p.Rcw[3 * a + b] = (double)Rcw(a, b); p.Rcb[3 * a + b] = (double)Rcb(a, b); }
            p.tcw[a] = (double)tcw(a); p.tcb[a] = (double)tcb(a); p.tbc[a] = (double)tbc(a);
        }
    }
    p.fx = pFrame->fx; p.fy = pFrame->fy; p.cx = pFrame->cx; p.cy = pFrame->cy; p.mbf = pFrame->mbf;
    typedef typename std::decay<decltype(*pFrame->mvpMapPoints[0])>::type MapPointT;
    const int N = pFrame->N;
    static thread_local std::vector<uint8_t> has, out, close, closeN;
    static thread_local std::vector<float> pos, xy, ur, inv;
    static thread_local std::vector<int> index;
    has.assign((size_t)N, 0);
    closeN.assign((size_t)N, 0);
    pos.resize(3 * (size_t)N);
    index.clear();
    {
        std::unique_lock<std::mutex> lock(MapPointT::mGlobalMutex);                                      // :4474
        for (int i = 0; i < N; i++) {
            const auto pMP = pFrame->mvpMapPoints[i];
            if (pMP) {                                                                                   // :4478: no isBad() here
                pFrame->mvbOutlier[i] = false;                                                           // :4489, :4517
                const auto Xw = pMP->GetWorldPos();
                has[i] = 1;
                closeN[i] = pMP->mTrackDepth < 10.f ? 1 : 0;                                             // :4657
                pos[3 * (size_t)i] = Xw(0); pos[3 * (size_t)i + 1] = Xw(1); pos[3 * (size_t)i + 2] = Xw(2);
                index.push_back(i);
            }
        }
    }
    p.n = (int)index.size();
    out.assign((size_t)N, 0);
    if (resident) {
        if (msorb_frame_pose_inertial_optimization(resident, &p, has.data(), pos.data(), closeN.data(), pFrame->mvInvLevelSigma2.data(),
                                                   (int)pFrame->mvInvLevelSigma2.size(), out.data(), &r) != MSORB_OK)
            fail_call("msorb_frame_pose_inertial_optimization");
        for (int i : index) pFrame->mvbOutlier[i] = out[i] != 0;
    } else {
        const size_t m = index.size();
        xy.resize(2 * m); ur.resize(m); inv.resize(m); close.resize(m);
        for (size_t k = 0; k < m; k++) {
            const int i = index[k];
            const auto& kpUn = pFrame->mvKeysUn[i];                                                      // :4486, :4519
            xy[2 * k] = kpUn.pt.x; xy[2 * k + 1] = kpUn.pt.y;
            ur[k] = pFrame->mvuRight[i];                                                                 // :4482, :4520
            inv[k] = pFrame->mvInvLevelSigma2[kpUn.octave];                                              // :4502 (uncertainty2 == 1 for Pinhole)
            close[k] = closeN[i];
            pos[3 * k] = pos[3 * (size_t)i]; pos[3 * k + 1] = pos[3 * (size_t)i + 1]; pos[3 * k + 2] = pos[3 * (size_t)i + 2];   // (k <= i)
        }
        const int off[2] = {0, (int)m};
        if (msorb_pose_inertial_optimization_batch(device, 1, &p, off, xy.data(), ur.data(), inv.data(), pos.data(), close.data(), out.data(), &r,
                                                   nullptr) != MSORB_OK)
            fail_call("msorb_pose_inertial_optimization_batch");
        for (size_t k = 0; k < m; k++) pFrame->mvbOutlier[index[k]] = out[k] != 0;
    }
    typedef typename std::decay<decltype(pFrame->GetImuRotation())>::type RotF;
    typedef typename std::decay<decltype(pFrame->GetImuPosition())>::type VecF;
    typedef typename std::decay<decltype(pFrame->GetVelocity())>::type VelF;
    RotF Rf;
    VecF tf;
    VelF vf;
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) Rf(a, b) = r.Rwb_f[3 * a + b];
        tf(a) = r.twb_f[a];
        vf(a) = r.v_f[a];
    }
    pFrame->SetImuPoseVelocity(Rf, tf, vf);                                                              // :4736-4737
    typedef typename std::decay<decltype(pFrame->mImuBias)>::type BiasT;
    pFrame->mImuBias = BiasT((float)r.est.ba[0], (float)r.est.ba[1], (float)r.est.ba[2], (float)r.est.bg[0], (float)r.est.bg[1],
                             (float)r.est.bg[2]);                                                        // :4738-4740
    typedef typename std::remove_pointer<typename std::decay<decltype(pFrame->mpcpi)>::type>::type ConstraintT;
    typedef typename std::decay<decltype(ConstraintT::Rwb)>::type RotD;
    typedef typename std::decay<decltype(ConstraintT::twb)>::type VecD;
    typedef typename std::decay<decltype(ConstraintT::H)>::type HessD;
    RotD Rd;
    VecD td, vd, bgd, bad;
    HessD Hd;
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) Rd(a, b) = r.est.Rwb[3 * a + b];
        td(a) = r.est.twb[a]; vd(a) = r.est.v[a]; bgd(a) = r.est.bg[a]; bad(a) = r.est.ba[a];
    }
    for (int a = 0; a < 15; a++)
        for (int b = 0; b < 15; b++) Hd(a, b) = r.H_prior[15 * a + b];
    pFrame->mpcpi = new ConstraintT(Rd, td, vd, bgd, bad, Hd);                                           // :4775-4776
    pFrame->mpcpi->H = Hd;                                                                               // (the constructor clipped it once more)
    if (form == 1) {
        delete pFp->mpcpi;                                                                               // :5168-5169
        pFp->mpcpi = NULL;
    }
    return r.n_initial - r.n_bad;                                                                        // :4778
}
}  // namespace pose_inertial_detail

template <class FrameT>
int PoseInertialOptimizationLastKeyFrame(FrameT* pFrame, msorb_frame* resident, bool bRecInit = false, int device = 0) {
    return pose_inertial_detail::Run(pFrame, 0, resident, bRecInit, device);
}
template <class FrameT>
int PoseInertialOptimizationLastKeyFrame(FrameT* pFrame, bool bRecInit = false) {
    return pose_inertial_detail::Run(pFrame, 0, static_cast<msorb_frame*>(nullptr), bRecInit, 0);
}
template <class FrameT>
int PoseInertialOptimizationLastFrame(FrameT* pFrame, msorb_frame* resident, bool bRecInit = false, int device = 0) {
    return pose_inertial_detail::Run(pFrame, 1, resident, bRecInit, device);
}
template <class FrameT>
int PoseInertialOptimizationLastFrame(FrameT* pFrame, bool bRecInit = false) {
    return pose_inertial_detail::Run(pFrame, 1, static_cast<msorb_frame*>(nullptr), bRecInit, 0);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Optimizer::LocalInertialBA (src/Optimizer.cc:2431-2973; LocalMapping.cc:150) on msorb_local_inertial_ba.
//
//   bool ORB_SLAM3::msorb_host::LocalInertialBA(pKF, pbStopFlag, pMap, num_fixedKF, num_OptKF, num_MPs, num_edges, bLarge, bRecInit)
//
// the reference's parameter list (pKF is its shared_ptr<KeyFrame>) and its effects: SetNewBias on the window's preintegrations
// (:2632), then under mMutexMapUpdate the flagged observations erased, mnBAFixedForKF / mnBALocalForKF reset, SetPose, SetVelocity,
// SetNewBias, SetWorldPos, UpdateNormalAndDepth, IncreaseChangeIndex (:2907-2972).  On the FAIL rule of :2911 it returns true with
// nothing written and the marks left as the reference leaves them.  The reference never assigns its four num_* outputs, nor does
// this.  *pbStopFlag is not read: the reference installs it after optimize() (:2868-2869).
//
// false = NOT handled, nothing touched, the caller runs Optimizer::LocalInertialBA: a KeyFrame with mpCamera2 anywhere in the
// problem (the arm :2820-2853), a window KeyFrame or the KeyFrame before the window that would take one of the reference's error
// branches (:2627-2630, :2642-2646, :2684-2685: !bImu, no mpImuPreintegrated), a covariance without inverse, more free KeyFrames
// than msorb_local_inertial_ba_capacity().  The decision falls before the first side effect: the chain is walked without a mark
// first, and the marks the gathering walk sets are put back before a late `false`; SetNewBias runs after the last check.
//
// The KeyFrames are handed over in ascending mnId, which is the order of g2o's unknowns (every free pose, then velocity and
// biases per KeyFrame).  Pinhole::uncertainty2 is 1.f, so inv_sigma2 is mvInvLevelSigma2[octave] / 1.f (:2771-2773).
template <class KFPtr, class MPPtr>
struct LocalInertialBAProblem : BaEdges {
    std::vector<KFPtr> vpOptimizableKFs;               // newest first, as the reference's
    std::list<KFPtr> lFixedKeyFrames;
    std::list<MPPtr> lLocalMapPoints;
    std::vector<KFPtr> kf_of_index;                    // ascending mnId
    std::vector<msorb_iba_keyframe> kfs;
    std::vector<msorb_iba_inertial_edge> iedges;       // in the order of the reference's loop (:2624-2686)
    std::vector<float> pos_w;
    std::vector<uint8_t> point_close;
    std::vector<std::pair<KFPtr, MPPtr>> edge_objects;
    bool handled = true;
    std::vector<std::pair<KFPtr, std::pair<unsigned long, unsigned long>>> kf_marks;
    std::vector<std::pair<MPPtr, unsigned long>> mp_marks;
    void restore_marks() {
        for (auto it = kf_marks.rbegin(); it != kf_marks.rend(); ++it) { it->first->mnBALocalForKF = it->second.first; it->first->mnBAFixedForKF = it->second.second; }
        for (auto it = mp_marks.rbegin(); it != mp_marks.rend(); ++it) it->first->mnBALocalForKF = it->second;
    }
};

template <class KFPtr>
msorb_iba_keyframe IbaKeyFrame(const KFPtr& k, int kind) {
    msorb_iba_keyframe r;
    std::memset(&r, 0, sizeof r);
    const auto Tcw = k->GetPose();                                                                       // G2oTypes.cc:95-100
    const auto Rcw = Tcw.rotationMatrix();
    const auto tcw = Tcw.translation();
    const auto Rwb = k->GetImuRotation();
    const auto twb = k->GetImuPosition();
    const auto Rcb = k->mImuCalib.mTcb.rotationMatrix();
    const auto tcb = k->mImuCalib.mTcb.translation();
    const auto tbc = k->mImuCalib.mTbc.translation();
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) { r.Rwb[3 * a + b] = (double)Rwb(a, b); r.Rcw[3 * a + b] = (double)Rcw(a, b); r.Rcb[3 * a + b] = (double)Rcb(a, b); }
        r.twb[a] = (double)twb(a); r.tcw[a] = (double)tcw(a); r.tcb[a] = (double)tcb(a); r.tbc[a] = (double)tbc(a);
    }
    if (kind != 2) {                                                                                     // VertexVelocity / GyroBias / AccBias(pKF)
        const auto v = k->GetVelocity();
        const auto bg = k->GetGyroBias();
        const auto ba = k->GetAccBias();
        for (int a = 0; a < 3; a++) { r.v[a] = (double)v(a); r.bg[a] = (double)bg(a); r.ba[a] = (double)ba(a); }
    }
    r.fx = k->fx; r.fy = k->fy; r.cx = k->cx; r.cy = k->cy; r.mbf = k->mbf;
    r.kind = kind;
    return r;
}

// :2441-2536 and :2624-2860.  B.handled == false: not handled; the marks are already put back.
template <class KFPtr, class MapT>
auto GatherLocalInertialBA(KFPtr pKF, MapT* pMap, bool bLarge, bool bRecInit) {
    (void)pMap;
    typedef typename std::decay<decltype(pKF->GetMapPointMatches()[0])>::type MPPtr;
    LocalInertialBAProblem<KFPtr, MPPtr> B;
    auto* pCurrentMap = pKF->GetMap();
    const int maxOpt = bLarge ? 25 : 10;                                                                 // :2435-2440
    const int Nd = std::min((int)pCurrentMap->KeyFramesInMap() - 2, maxOpt);
    // ---- the chain, without a mark: everything that can be refused from it is refused here
    std::vector<KFPtr> chain;
    chain.push_back(pKF);
    for (int i = 1; i < Nd; i++) {
        if (!chain.back()->mPrevKF) break;
        chain.push_back(chain.back()->mPrevKF);
    }
    const bool has_prev = (bool)chain.back()->mPrevKF;
    const KFPtr first_fixed = has_prev ? chain.back()->mPrevKF : chain.back();
    const size_t N = has_prev ? chain.size() : chain.size() - 1;                                         // :2480-2488
    auto refuse = [&] { B.handled = false; return B; };
    if ((int)N > msorb_local_inertial_ba_capacity()) return refuse();
    if (first_fixed->mpCamera2 || (N > 0 && !first_fixed->bImu)) return refuse();                        // :2602, :2642-2646
    for (size_t i = 0; i < N; i++) {
        const KFPtr& k = chain[i];
        if (k->mpCamera2 || !k->bImu || !k->mPrevKF || !k->mpImuPreintegrated) return refuse();          // :2568, :2627-2630, :2684-2685
    }
    // ---- the reference's walk, with its marks
    auto mark = [&](const KFPtr& k) { B.kf_marks.push_back({k, {k->mnBALocalForKF, k->mnBAFixedForKF}}); };
    for (size_t i = 0; i < chain.size(); i++) {                                                          // :2449-2457
        mark(chain[i]);
        chain[i]->mnBALocalForKF = pKF->mnId;
        B.vpOptimizableKFs.push_back(chain[i]);
    }
    for (const KFPtr& k : B.vpOptimizableKFs) {                                                          // :2465-2476
        const auto vpMPs = k->GetMapPointMatches();
        for (const MPPtr& pMP : vpMPs)
            if (pMP && !pMP->isBad() && pMP->mnBALocalForKF != pKF->mnId) {
                B.lLocalMapPoints.push_back(pMP);
                B.mp_marks.push_back({pMP, pMP->mnBALocalForKF});
                pMP->mnBALocalForKF = pKF->mnId;
            }
    }
    if (has_prev) {                                                                                      // :2480-2488
        mark(first_fixed);
        first_fixed->mnBAFixedForKF = pKF->mnId;
    } else {
        first_fixed->mnBALocalForKF = 0;
        first_fixed->mnBAFixedForKF = pKF->mnId;
        B.vpOptimizableKFs.pop_back();
    }
    B.lFixedKeyFrames.push_back(first_fixed);
    // (lpOptVisKFs: maxCovKF = 0 keeps it empty, :2491-2514)
    bool two_cameras = false;
    for (const MPPtr& pMP : B.lLocalMapPoints) {                                                         // :2519-2536
        const auto observations = pMP->GetObservations();
        for (const auto& ob : observations) {
            KFPtr pKFi = ob.first;
            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                mark(pKFi);
                pKFi->mnBAFixedForKF = pKF->mnId;
                if (!pKFi->isBad()) {
                    B.lFixedKeyFrames.push_back(pKFi);
                    if (pKFi->mpCamera2) two_cameras = true;
                    break;
                }
            }
        }
        if (B.lFixedKeyFrames.size() >= 200) break;
    }
    // ---- the vertices, ascending mnId (:2559-2617)
    std::map<unsigned long, std::pair<KFPtr, int>> by_id;
    for (const KFPtr& k : B.vpOptimizableKFs) by_id[k->mnId] = {k, 0};
    for (const KFPtr& k : B.lFixedKeyFrames) by_id[k->mnId] = {k, k->bImu ? 1 : 2};                      // :2602
    std::map<KFPtr, int> index;
    for (const auto& it : by_id) {
        index[it.second.first] = (int)B.kfs.size();
        B.kfs.push_back(IbaKeyFrame(it.second.first, it.second.second));
        B.kf_of_index.push_back(it.second.first);
    }
    // ---- the inertial edges (:2624-2686); the bias SetNewBias will install is mPrevKF->GetImuBias(), read here, set by the caller
    const int Nw = (int)B.vpOptimizableKFs.size();
    for (int i = 0; i < Nw && !two_cameras; i++) {
        const KFPtr& k = B.vpOptimizableKFs[i];
        msorb_iba_inertial_edge e;
        std::memset(&e, 0, sizeof e);
        const auto pInt = k->mpImuPreintegrated;
        if (!pose_inertial_detail::EdgeOf(pInt, e.pre) || !pose_inertial_detail::RandomWalkInformation(pInt, 9, e.info_gyro) ||
            !pose_inertial_detail::RandomWalkInformation(pInt, 12, e.info_acc)) {
            two_cameras = true;   // (refused below like a late second camera)
            break;
        }
        e.pre.kf_prev = index[k->mPrevKF];
        e.pre.kf_cur = index[k];
        e.huber = (i == Nw - 1 || bRecInit) ? 1 : 0;                                                     // :2657-2667
        e.downweight = i == Nw - 1 ? 1 : 0;
        B.iedges.push_back(e);
    }
    if (two_cameras) {
        B.restore_marks();
        return refuse();
    }
    // ---- the points and the visual edges (:2729-2856)
    int nPoints = 0;
    for (const MPPtr& pMP : B.lLocalMapPoints) {
        const auto Xw = pMP->GetWorldPos();
        B.pos_w.push_back(Xw(0)); B.pos_w.push_back(Xw(1)); B.pos_w.push_back(Xw(2));
        B.point_close.push_back(pMP->mTrackDepth < 10.f ? 1 : 0);                                        // :2879
        const auto observations = pMP->GetObservations();
        for (const auto& ob : observations) {
            KFPtr pKFi = ob.first;
            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) continue;        // :2746
            if (pKFi->isBad() || pKFi->GetMap() != pCurrentMap) continue;                                // :2749
            const auto at = index.find(pKFi);
            if (at == index.end()) continue;   // (marked fixed but bad: no vertex; the reference's setVertex would get NULL)
            if (B.append(pKFi, std::get<0>(ob.second), at->second, nPoints)) B.edge_objects.push_back({pKFi, pMP});
        }
        nPoints++;
    }
    return B;
}

template <class KFPtr, class MapT>
bool LocalInertialBA(KFPtr pKF, bool* pbStopFlag, MapT* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs, int& num_edges,
                     bool bLarge = false, bool bRecInit = false, int device = 0) {
    (void)pbStopFlag; (void)num_fixedKF; (void)num_OptKF; (void)num_MPs; (void)num_edges;
    auto B = GatherLocalInertialBA(pKF, pMap, bLarge, bRecInit);
    if (!B.handled) return false;
    const int K = (int)B.kfs.size(), P = (int)B.lLocalMapPoints.size(), E = (int)B.edge_kf.size(), NI = (int)B.iedges.size();
    msorb_iba_problem prob;
    std::memset(&prob, 0, sizeof prob);
    prob.large = bLarge ? 1 : 0;
    std::vector<msorb_iba_keyframe_out> kf_out((size_t)K);
    std::vector<float> pos_out(3 * (size_t)P);
    std::vector<uint8_t> outlier((size_t)E);
    msorb_iba_result r;
    const int rc = msorb_local_inertial_ba(device, &prob, K, B.kfs.data(), NI, B.iedges.data(), P, B.pos_w.data(), B.point_close.data(), E,
                                           B.edge_kf.data(), B.edge_point.data(), B.xy.data(), B.u_right.data(), B.inv_sigma2.data(),
                                           kf_out.data(), pos_out.data(), nullptr, outlier.data(), &r, nullptr);
    if (rc == MSORB_E_CAPACITY) { B.restore_marks(); return false; }
    if (rc != MSORB_OK) fail_call("msorb_local_inertial_ba");
    for (const KFPtr& k : B.vpOptimizableKFs) k->mpImuPreintegrated->SetNewBias(k->mPrevKF->GetImuBias());   // :2632
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                                            // :2907
    if (r.status == 1) return true;                                                                      // :2911-2915
    for (int pass = 0; pass < 2; pass++)                                                                 // vToErase: the mono edges, then the stereo edges
        for (int e = 0; e < E; e++) {
            if (!outlier[e] || (B.u_right[e] >= 0) != (pass == 1)) continue;
            const auto& o = B.edge_objects[e];
            if (o.second->isBad()) continue;                                                             // :2881, :2897
            o.first->EraseMapPointMatch(o.second);                                                       // :2922-2923
            o.second->EraseObservation(o.first);
        }
    for (const KFPtr& k : B.lFixedKeyFrames) k->mnBAFixedForKF = 0;                                      // :2927-2928
    typedef typename std::decay<decltype(pKF->GetPose())>::type SE3T;
    typedef typename std::decay<decltype(pKF->GetPose().rotationMatrix())>::type RotF;
    typedef typename std::decay<decltype(pKF->GetPose().translation())>::type VecF;
    typedef typename std::decay<decltype(pKF->GetVelocity())>::type VelF;
    typedef typename std::decay<decltype(pKF->GetImuBias())>::type BiasT;
    std::map<KFPtr, int> index;
    for (int k = 0; k < K; k++) index[B.kf_of_index[k]] = k;
    for (const KFPtr& k : B.vpOptimizableKFs) {                                                          // :2933-2951
        const msorb_iba_keyframe_out& o = kf_out[index[k]];
        RotF Rf;
        VecF tf;
        VelF vf;
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) Rf(a, b) = o.Rcw_f[3 * a + b];
            tf(a) = o.tcw_f[a];
            vf(a) = o.v_f[a];
        }
        k->SetPose(SE3T(Rf, tf));
        k->mnBALocalForKF = 0;
        k->SetVelocity(vf);
        k->SetNewBias(BiasT(o.bias_f[0], o.bias_f[1], o.bias_f[2], o.bias_f[3], o.bias_f[4], o.bias_f[5]));
    }
    typedef typename std::decay<decltype(B.lLocalMapPoints.front()->GetWorldPos())>::type PosT;
    int p = 0;
    for (const auto& pMP : B.lLocalMapPoints) {                                                          // :2963-2970
        const float* o = pos_out.data() + 3 * (size_t)p++;
        pMP->SetWorldPos(PosT(o[0], o[1], o[2]));
        pMP->UpdateNormalAndDepth();
    }
    pMap->IncreaseChangeIndex();                                                                         // :2972
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Optimizer::FullInertialBA (src/Optimizer.cc:366-756; LocalMapping.cc:1328, :1330, LoopClosing.cc:2230) on msorb_full_inertial_ba.
//
//   bool ORB_SLAM3::msorb_host::FullInertialBA(pMap, its, bFixLocal, nLoopId, pbStopFlag, bInit, priorG, priorA, vSingVal, bHess)
//
// the reference's parameter list and defaults (vSingVal and bHess are unused by the reference and unused here) and its effects:
// SetNewBias(mPrevKF->GetImuBias()) on the preintegration of every inertial link (:456), then for every KeyFrame up to GetMaxKFid()
// with nLoopId == 0 SetPose / SetVelocity / SetNewBias, otherwise mTcwGBA / mVwbGBA / mBiasGBA and mnBAGlobalForKF; for every point
// that is a vertex SetWorldPos + UpdateNormalAndDepth, otherwise mPosGBA and mnBAGlobalForKF; IncreaseChangeIndex.  true = done,
// including bFixLocal's nNonFixed < 3 return (:438-441, nothing touched) and the stop flag found set before optimize() (:683-685,
// after the SetNewBias of :456 and before any write-back, as in the reference).
//
// false = NOT handled, nothing touched, the caller runs Optimizer::FullInertialBA: a KeyFrame with mpCamera2 (the arm :643-673), a
// free KeyFrame without bImu, an inertial link without mpImuPreintegrated or whose covariance has no inverse, links that are no
// chains (two KeyFrames with one mPrevKF), more free KeyFrames than msorb_full_inertial_ba_capacity(bInit), or a call in which a
// factorisation of the reduced system met a pivot that was not positive (msorb_iba_result::reserved; a large map without a fixed
// KeyFrame under lambda = 1e-5: the dense unpivoted solve cannot stand in for the reference's there).  The decision falls before the
// first side effect: SetNewBias runs after the call has been accepted.
//
// The KeyFrames are handed over in ascending mnId (g2o's order of the unknowns), the inertial edges in the order of the reference's
// loop over GetAllKeyFrames(), the points in the order of GetAllMapPoints().  With bInit the shared biases start at those of the
// last KeyFrame the vertex loop visits (pIncKF, :399, :428-435).
template <class KFPtr, class MPPtr>
struct FullInertialBAProblem : BaEdges {
    std::vector<KFPtr> vpKFs;                          // GetAllKeyFrames() up to maxKFid, in its order
    std::vector<MPPtr> vpMPs;
    std::vector<KFPtr> kf_of_index;                    // ascending mnId
    std::vector<msorb_iba_keyframe> kfs;
    std::vector<msorb_iba_inertial_edge> iedges;
    std::vector<KFPtr> new_bias;                       // the KeyFrames whose preintegration receives SetNewBias (:456), in order
    std::vector<float> pos_w;
    msorb_fiba_problem prob;
    bool handled = true, too_few = false;              // too_few: nNonFixed < 3
};

template <class MapT>
auto GatherFullInertialBA(MapT* pMap, int its, bool bFixLocal, bool bInit, float priorG, float priorA) {
    const auto all = pMap->GetAllKeyFrames();
    const auto vpMPs = pMap->GetAllMapPoints();
    typedef typename std::decay<decltype(all[0])>::type KFPtr;
    typedef typename std::decay<decltype(vpMPs[0])>::type MPPtr;
    FullInertialBAProblem<KFPtr, MPPtr> B;
    std::memset(&B.prob, 0, sizeof B.prob);
    B.prob.init = bInit ? 1 : 0;
    B.prob.iterations = its;
    B.prob.prior_g = priorG;
    B.prob.prior_a = priorA;
    const unsigned long maxKFid = pMap->GetMaxKFid();
    auto refuse = [&] { B.handled = false; return B; };
    // ---- the vertices (:393-441)
    int nNonFixed = 0;
    std::map<unsigned long, std::pair<KFPtr, int>> by_id;
    KFPtr pIncKF;
    for (const KFPtr& pKFi : all) {
        if (pKFi->mnId > maxKFid) continue;
        B.vpKFs.push_back(pKFi);
        pIncKF = pKFi;
        bool bFixed = false;
        if (bFixLocal) {
            bFixed = (pKFi->mnBALocalForKF >= (maxKFid - 1)) || (pKFi->mnBAFixedForKF >= (maxKFid - 1));
            if (!bFixed) nNonFixed++;
        }
        if (pKFi->mpCamera2) return refuse();
        if (!bFixed && !pKFi->bImu) return refuse();
        by_id[pKFi->mnId] = {pKFi, bFixed ? (pKFi->bImu ? 1 : 2) : 0};
    }
    if (bFixLocal && nNonFixed < 3) { B.too_few = true; return B; }
    std::map<KFPtr, int> index;
    for (const auto& it : by_id) {
        index[it.second.first] = (int)B.kfs.size();
        B.kfs.push_back(IbaKeyFrame(it.second.first, it.second.second));
        B.kf_of_index.push_back(it.second.first);
    }
    if (bInit && pIncKF) {
        const auto bg = pIncKF->GetGyroBias();
        const auto ba = pIncKF->GetAccBias();
        for (int a = 0; a < 3; a++) { B.prob.bg0[a] = (double)bg(a); B.prob.ba0[a] = (double)ba(a); }
    }
    // ---- the inertial links (:444-526)
    for (const KFPtr& pKFi : all) {
        if (!pKFi->mPrevKF || pKFi->mnId > maxKFid) continue;
        if (pKFi->isBad() || pKFi->mPrevKF->mnId > maxKFid) continue;
        if (!(pKFi->bImu && pKFi->mPrevKF->bImu)) continue;                                                    // :523-524
        if (!pKFi->mpImuPreintegrated) return refuse();
        B.new_bias.push_back(pKFi);                                                                         // :456
        const auto prev = index.find(pKFi->mPrevKF);
        if (prev == index.end()) continue;                                                               // :478-489: a vertex is missing
        msorb_iba_inertial_edge e;
        std::memset(&e, 0, sizeof e);
        if (!pose_inertial_detail::EdgeOf(pKFi->mpImuPreintegrated, e.pre)) return refuse();
        if (!bInit && (!pose_inertial_detail::RandomWalkInformation(pKFi->mpImuPreintegrated, 9, e.info_gyro) ||
                       !pose_inertial_detail::RandomWalkInformation(pKFi->mpImuPreintegrated, 12, e.info_acc)))
            return refuse();
        e.pre.kf_prev = prev->second;
        e.pre.kf_cur = index[pKFi];
        e.huber = 1;                                                                                     // :499-501
        e.downweight = 0;
        B.iedges.push_back(e);
    }
    // ---- the points and the visual edges (:556-681)
    int nPoints = 0;
    for (const MPPtr& pMP : vpMPs) {
        B.vpMPs.push_back(pMP);
        const auto Xw = pMP->GetWorldPos();
        B.pos_w.push_back(Xw(0)); B.pos_w.push_back(Xw(1)); B.pos_w.push_back(Xw(2));
        const auto observations = pMP->GetObservations();
        for (const auto& ob : observations) {
            KFPtr pKFi = ob.first;
            if (pKFi->mnId > maxKFid || pKFi->isBad()) continue;
            const auto at = index.find(pKFi);
            if (at == index.end()) continue;
            B.append(pKFi, std::get<0>(ob.second), at->second, nPoints);
        }
        nPoints++;
    }
    return B;
}

template <class MapT, class VecT = void>
bool FullInertialBA(MapT* pMap, int its, const bool bFixLocal = false, const unsigned long nLoopId = 0, bool* pbStopFlag = nullptr,
                    bool bInit = false, float priorG = 1e2, float priorA = 1e6, VecT* vSingVal = nullptr, bool* bHess = nullptr, int device = 0) {
    (void)vSingVal; (void)bHess;
    auto B = GatherFullInertialBA(pMap, its, bFixLocal, bInit, priorG, priorA);
    if (!B.handled) return false;
    if (B.too_few) return true;                                                                          // :438-441
    const int K = (int)B.kfs.size(), P = (int)B.vpMPs.size(), E = (int)B.edge_kf.size(), NI = (int)B.iedges.size();
    std::vector<msorb_iba_keyframe_out> kf_out((size_t)K);
    std::vector<float> pos_out(3 * (size_t)P);
    std::vector<uint8_t> included((size_t)P);
    msorb_iba_result r;
    int rc;
    {
        StopFlagMirror stop(pbStopFlag);
        rc = msorb_full_inertial_ba(device, &B.prob, K, B.kfs.data(), NI, B.iedges.data(), P, B.pos_w.data(), E, B.edge_kf.data(),
                                    B.edge_point.data(), B.xy.data(), B.u_right.data(), B.inv_sigma2.data(), stop.get(), kf_out.data(),
                                    pos_out.data(), nullptr, included.data(), &r, nullptr);
    }
    if (rc == MSORB_E_CAPACITY) return false;
    if (rc != MSORB_OK) fail_call("msorb_full_inertial_ba");
    if (r.status == 0 && r.reserved != 0) return false;   // a factorisation failed: rounding decided the outcome, nothing touched yet
    for (const auto& pKFi : B.new_bias) pKFi->mpImuPreintegrated->SetNewBias(pKFi->mPrevKF->GetImuBias());        // :456
    if (r.status != 0) return true;                                                                      // :683-685: no write-back
    typedef typename std::decay<decltype(B.vpKFs[0])>::type KFPtr;
    typedef typename std::decay<decltype(B.vpKFs[0]->GetPose())>::type SE3T;
    typedef typename std::decay<decltype(B.vpKFs[0]->GetPose().rotationMatrix())>::type RotF;
    typedef typename std::decay<decltype(B.vpKFs[0]->GetPose().translation())>::type VecF;
    typedef typename std::decay<decltype(B.vpKFs[0]->GetVelocity())>::type VelF;
    typedef typename std::decay<decltype(B.vpKFs[0]->GetImuBias())>::type BiasT;
    std::map<KFPtr, int> index;
    for (int k = 0; k < K; k++) index[B.kf_of_index[k]] = k;
    for (const KFPtr& pKFi : B.vpKFs) {                                                                     // :694-734
        const msorb_iba_keyframe_out& o = kf_out[index[pKFi]];
        RotF Rf;
        VecF tf;
        VelF vf;
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) Rf(a, b) = o.Rcw_f[3 * a + b];
            tf(a) = o.tcw_f[a];
            vf(a) = o.v_f[a];
        }
        if (nLoopId == 0) pKFi->SetPose(SE3T(Rf, tf));
        else { pKFi->mTcwGBA = SE3T(Rf, tf); pKFi->mnBAGlobalForKF = nLoopId; }
        if (!pKFi->bImu) continue;
        const BiasT b(o.bias_f[0], o.bias_f[1], o.bias_f[2], o.bias_f[3], o.bias_f[4], o.bias_f[5]);
        if (nLoopId == 0) { pKFi->SetVelocity(vf); pKFi->SetNewBias(b); }
        else { pKFi->mVwbGBA = vf; pKFi->mBiasGBA = b; }
    }
    if (P) {
        typedef typename std::decay<decltype(B.vpMPs[0]->GetWorldPos())>::type PosT;
        for (int p = 0; p < P; p++) {                                                                    // :737-753
            if (!included[p]) continue;
            const float* o = pos_out.data() + 3 * (size_t)p;
            const auto& pMP = B.vpMPs[p];
            if (nLoopId == 0) { pMP->SetWorldPos(PosT(o[0], o[1], o[2])); pMP->UpdateNormalAndDepth(); }
            else { pMP->mPosGBA = PosT(o[0], o[1], o[2]); pMP->mnBAGlobalForKF = nLoopId; }
        }
    }
    pMap->IncreaseChangeIndex();                                                                         // :755
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Optimizer::MergeInertialBA (src/Optimizer.cc:3918-4420; LoopClosing.cc:1567, :1995) on msorb_merge_inertial_ba.
//
//   bool ORB_SLAM3::msorb_host::MergeInertialBA(pCurrKF, pMergeKF, pbStopFlag, pMap, corrPoses)
//
// the reference's parameter list and its effects: the marks of the gathering walk, SetNewBias(mPrevKF->GetImuBias()) on the
// preintegration of every inertial link (:4142), the flagged observations erased, then for both windows and for the covisible
// KeyFrames SetPose, corrPoses[pKFi] = Sim3(GetPose() widened, 1.0) and, with bImu, SetVelocity / SetNewBias (acc, then gyro); for
// every local point SetWorldPos + UpdateNormalAndDepth; IncreaseChangeIndex.  true = done, including the stop flag found set before
// optimize() (:4312-4314: after the marks and the SetNewBias of :4142, before any write-back, as in the reference).
//
// false = NOT handled, nothing touched (the marks are put back), the caller runs Optimizer::MergeInertialBA: a KeyFrame with
// mpCamera2; a window KeyFrame with mPrevKF for which the reference would print its error (no bImu on either end, no
// mpImuPreintegrated, a covariance without inverse, mPrevKF not among the vertices); vertex ids that would collide in g2o (a
// gathered KeyFrame with mnId > maxKFid, a KeyFrame gathered twice, maxKFid <= 2: the ids are mnId, maxKFid + 3 mnId + 1..3 and
// 5 maxKFid + mnId + 1); links that are no chains or more unknowns than msorb_merge_inertial_ba_capacity(); nothing to optimise; a
// call in which a factorisation met a pivot that was not positive (msorb_iba_result::reserved); and a flag that rose after the
// gathering and before the first iteration (status 3 without the flag having been set here: the reference would classify errors
// that were never computed).
//
// A KeyFrame's kind follows g2o's active set: free with an inertial edge at it = 0, free without = 3 (its velocity and bias
// vertices are in the reference's graph but no edge reaches them), fixed = 1 with bImu, else 2.  The KeyFrames are handed over in
// ascending mnId (g2o's order of the unknowns: every pose id is below every velocity / bias id), the inertial edges in the order of
// the loop over vpOptimizableKFs, the points in the order of lLocalMapPoints.
template <class KFPtr, class MPPtr>
struct MergeInertialBAProblem : BaEdges {
    std::vector<KFPtr> vpOptimizableKFs, vpOptimizableCovKFs;
    std::list<KFPtr> lFixedKeyFrames;
    std::list<MPPtr> lLocalMapPoints;
    std::vector<KFPtr> kf_of_index;                    // ascending mnId
    std::vector<msorb_iba_keyframe> kfs;
    std::vector<msorb_iba_inertial_edge> iedges;
    std::vector<KFPtr> new_bias;                       // the KeyFrames whose preintegration receives SetNewBias (:4142), in order
    std::vector<float> pos_w;
    std::vector<std::pair<KFPtr, MPPtr>> edge_objects;
    bool handled = true;
    std::vector<std::pair<KFPtr, std::pair<unsigned long, unsigned long>>> kf_marks;
    std::vector<std::pair<MPPtr, unsigned long>> mp_marks;
    void restore_marks() {
        for (auto it = kf_marks.rbegin(); it != kf_marks.rend(); ++it) { it->first->mnBALocalForKF = it->second.first; it->first->mnBAFixedForKF = it->second.second; }
        for (auto it = mp_marks.rbegin(); it != mp_marks.rend(); ++it) it->first->mnBALocalForKF = it->second;
    }
};

// :3920-4037 and the edge loops :4133-4307.  B.handled == false: not handled; the marks are already put back.
template <class KFPtr>
auto GatherMergeInertialBA(KFPtr pCurrKF, KFPtr pMergeKF) {
    typedef typename std::decay<decltype(pCurrKF->GetMapPointMatches()[0])>::type MPPtr;
    MergeInertialBAProblem<KFPtr, MPPtr> B;
    const int Nd = 6;
    const unsigned long maxKFid = pCurrKF->mnId, id = pCurrKF->mnId;
    const size_t maxCovKF = 30;
    auto refuse = [&] { B.restore_marks(); B.handled = false; return B; };
    auto mark = [&](const KFPtr& k) { B.kf_marks.push_back({k, {k->mnBALocalForKF, k->mnBAFixedForKF}}); };
    auto local = [&](const KFPtr& k) { mark(k); k->mnBALocalForKF = id; };
    auto& opt = B.vpOptimizableKFs;
    opt.push_back(pCurrKF);                                                                              // :3932-3940
    local(pCurrKF);
    for (int i = 1; i < Nd; i++) {
        if (!opt.back()->mPrevKF) break;
        opt.push_back(opt.back()->mPrevKF);
        local(opt.back());
    }
    if (opt.back()->mPrevKF) {                                                                           // :3943-3949
        B.vpOptimizableCovKFs.push_back(opt.back()->mPrevKF);
        local(opt.back()->mPrevKF);
    } else {
        B.vpOptimizableCovKFs.push_back(opt.back());
        opt.pop_back();
    }
    opt.push_back(pMergeKF);                                                                             // :3952-3962
    local(pMergeKF);
    for (int i = 1; i < Nd / 2; i++) {
        if (!opt.back()->mPrevKF) break;
        opt.push_back(opt.back()->mPrevKF);
        local(opt.back());
    }
    if (opt.back()->mPrevKF) {                                                                           // :3965-3973
        B.lFixedKeyFrames.push_back(opt.back()->mPrevKF);
        mark(opt.back()->mPrevKF);
        opt.back()->mPrevKF->mnBAFixedForKF = id;
    } else {
        mark(opt.back());
        opt.back()->mnBALocalForKF = 0;
        opt.back()->mnBAFixedForKF = id;
        B.lFixedKeyFrames.push_back(opt.back());
        opt.pop_back();
    }
    if (pMergeKF->mNextKF) {                                                                             // :3976-3987
        opt.push_back(pMergeKF->mNextKF);
        local(opt.back());
    }
    while (!opt.empty() && opt.size() < (size_t)(2 * Nd)) {
        const KFPtr pKFlast = opt.back();
        if (!pKFlast->mNextKF) break;
        opt.push_back(pKFlast->mNextKF);
        local(opt.back());
    }
    const int N = (int)opt.size();
    std::map<MPPtr, int> mLocalObs;                                                                      // :3992-4009
    for (int i = 0; i < N; i++) {
        const auto vpMPs = opt[i]->GetMapPointMatches();
        for (const MPPtr& pMP : vpMPs) {
            if (!pMP || pMP->isBad()) continue;
            if (pMP->mnBALocalForKF != id) {
                mLocalObs[pMP] = 1;
                B.lLocalMapPoints.push_back(pMP);
                B.mp_marks.push_back({pMP, pMP->mnBALocalForKF});
                pMP->mnBALocalForKF = id;
            } else
                mLocalObs[pMP]++;
        }
    }
    std::vector<std::pair<MPPtr, int>> pairs(mLocalObs.begin(), mLocalObs.end());                         // :4011-4015
    std::sort(pairs.begin(), pairs.end(), [](const std::pair<MPPtr, int>& a, const std::pair<MPPtr, int>& b) { return a.second < b.second; });
    size_t i_pair = 0;
    for (auto lit = pairs.begin(); lit != pairs.end(); ++lit, ++i_pair) {                                // :4018-4037
        const auto observations = lit->first->GetObservations();
        if (i_pair >= maxCovKF) break;
        for (const auto& ob : observations) {
            KFPtr pKFi = ob.first;
            if (pKFi->mnBALocalForKF != id && pKFi->mnBAFixedForKF != id) {
                local(pKFi);
                if (!pKFi->isBad()) {
                    B.vpOptimizableCovKFs.push_back(pKFi);
                    break;
                }
            }
        }
    }
    // ---- the vertices (:4052-4127): ascending mnId; what g2o would refuse or number twice is not handled
    if (maxKFid <= 2) return refuse();
    std::map<unsigned long, std::pair<KFPtr, int>> by_id;   // second: 0 free, 1 fixed
    auto add = [&](const KFPtr& k, int fixed) {
        if (k->mpCamera2 || k->mnId > maxKFid || by_id.count(k->mnId)) return false;
        by_id[k->mnId] = {k, fixed};
        return true;
    };
    for (const KFPtr& k : opt)
        if (!add(k, 0)) return refuse();
    for (const KFPtr& k : B.vpOptimizableCovKFs)
        if (!add(k, 0)) return refuse();
    for (const KFPtr& k : B.lFixedKeyFrames)
        if (!add(k, 1)) return refuse();
    std::map<KFPtr, int> index;
    for (const auto& it : by_id) {
        index[it.second.first] = (int)B.kf_of_index.size();
        B.kf_of_index.push_back(it.second.first);
    }
    // ---- the inertial edges (:4133-4188)
    std::vector<char> inertial(B.kf_of_index.size(), 0);
    for (int i = 0; i < N; i++) {
        const KFPtr& k = opt[i];
        if (!k->mPrevKF) continue;                                                                       // :4137-4140
        if (!(k->bImu && k->mPrevKF->bImu && k->mpImuPreintegrated)) return refuse();                    // :4186-4187
        const auto prev = index.find(k->mPrevKF);
        if (prev == index.end()) return refuse();                                                        // :4152-4156
        msorb_iba_inertial_edge e;
        std::memset(&e, 0, sizeof e);
        if (!pose_inertial_detail::EdgeOf(k->mpImuPreintegrated, e.pre) || !pose_inertial_detail::RandomWalkInformation(k->mpImuPreintegrated, 9, e.info_gyro) ||
            !pose_inertial_detail::RandomWalkInformation(k->mpImuPreintegrated, 12, e.info_acc))
            return refuse();
        e.pre.kf_prev = prev->second;
        e.pre.kf_cur = index[k];
        e.huber = 1;                                                                                     // :4168-4170
        e.downweight = 0;
        inertial[e.pre.kf_prev] = inertial[e.pre.kf_cur] = 1;
        B.iedges.push_back(e);
        B.new_bias.push_back(k);                                                                         // :4142
    }
    for (size_t k = 0; k < B.kf_of_index.size(); k++) {
        const KFPtr& pKFi = B.kf_of_index[k];
        const bool fixed = by_id[pKFi->mnId].second != 0;
        // (a kind 3 record carries the velocity and the biases the write-back hands back unchanged, :4398-4406)
        B.kfs.push_back(IbaKeyFrame(pKFi, fixed ? (pKFi->bImu ? 1 : 2) : (inertial[k] ? 0 : 3)));
    }
    // ---- the points and the visual edges (:4223-4307)
    int nPoints = 0;
    for (const MPPtr& pMP : B.lLocalMapPoints) {
        const auto Xw = pMP->GetWorldPos();
        B.pos_w.push_back(Xw(0)); B.pos_w.push_back(Xw(1)); B.pos_w.push_back(Xw(2));
        const auto observations = pMP->GetObservations();
        for (const auto& ob : observations) {
            KFPtr pKFi = ob.first;
            if (!pKFi) continue;
            if (pKFi->mnBALocalForKF != id && pKFi->mnBAFixedForKF != id) continue;                      // :4247
            if (pKFi->mnId > maxKFid) continue;                                                          // :4250
            const auto at = index.find(pKFi);
            if (at == index.end() || pKFi->isBad()) continue;                                            // :4255, :4258
            if (B.append(pKFi, std::get<0>(ob.second), at->second, nPoints)) B.edge_objects.push_back({pKFi, pMP});
        }
        nPoints++;
    }
    return B;
}

template <class KFPtr, class MapT, class CorrT>
bool MergeInertialBA(KFPtr pCurrKF, KFPtr pMergeKF, bool* pbStopFlag, MapT* pMap, CorrT& corrPoses, int device = 0) {
    auto B = GatherMergeInertialBA(pCurrKF, pMergeKF);
    if (!B.handled) return false;
    auto set_new_bias = [&] {
        for (const auto& k : B.new_bias) k->mpImuPreintegrated->SetNewBias(k->mPrevKF->GetImuBias());    // :4142
    };
    if (pbStopFlag && *pbStopFlag) {                                                                     // :4312-4314
        set_new_bias();
        return true;
    }
    const int K = (int)B.kfs.size(), P = (int)B.lLocalMapPoints.size(), E = (int)B.edge_kf.size(), NI = (int)B.iedges.size();
    msorb_iba_problem prob;
    std::memset(&prob, 0, sizeof prob);
    std::vector<msorb_iba_keyframe_out> kf_out((size_t)K);
    std::vector<float> pos_out(3 * (size_t)P);
    std::vector<uint8_t> outlier((size_t)E), included((size_t)P);
    msorb_iba_result r;
    int rc;
    {
        StopFlagMirror stop(pbStopFlag);
        rc = msorb_merge_inertial_ba(device, &prob, K, B.kfs.data(), NI, B.iedges.data(), P, B.pos_w.data(), E, B.edge_kf.data(),
                                     B.edge_point.data(), B.xy.data(), B.u_right.data(), B.inv_sigma2.data(), stop.get(), kf_out.data(),
                                     pos_out.data(), nullptr, outlier.data(), included.data(), &r, nullptr);
    }
    if (rc != MSORB_OK && rc != MSORB_E_CAPACITY) fail_call("msorb_merge_inertial_ba");
    // no chains or too large; nothing to optimise; the flag rose before the first iteration; a factorisation failed
    if (rc == MSORB_E_CAPACITY || r.status != 0 || r.reserved != 0) { B.restore_marks(); return false; }
    set_new_bias();
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                                            // :4352
    for (int pass = 0; pass < 2; pass++)                                                                 // vToErase: the mono edges, then the stereo edges
        for (int e = 0; e < E; e++) {
            if (!outlier[e] || (B.u_right[e] >= 0) != (pass == 1)) continue;
            const auto& o = B.edge_objects[e];
            if (o.second->isBad()) continue;                                                             // :4328, :4342
            o.first->EraseMapPointMatch(o.second);                                                       // :4357-4358
            o.second->EraseObservation(o.first);
        }
    typedef typename std::decay<decltype(pCurrKF->GetPose())>::type SE3T;
    typedef typename std::decay<decltype(pCurrKF->GetPose().rotationMatrix())>::type RotF;
    typedef typename std::decay<decltype(pCurrKF->GetPose().translation())>::type VecF;
    typedef typename std::decay<decltype(pCurrKF->GetVelocity())>::type VelF;
    typedef typename std::decay<decltype(pCurrKF->GetImuBias())>::type BiasT;
    typedef typename CorrT::mapped_type Sim3T;
    std::map<KFPtr, int> index;
    for (int k = 0; k < K; k++) index[B.kf_of_index[k]] = k;
    for (const auto* list : {&B.vpOptimizableKFs, &B.vpOptimizableCovKFs})                               // :4365-4385, :4387-4407
        for (const KFPtr& pKFi : *list) {
            const msorb_iba_keyframe_out& o = kf_out[index[pKFi]];
            RotF Rf;
            VecF tf;
            VelF vf;
            for (int a = 0; a < 3; a++) {
                for (int b = 0; b < 3; b++) Rf(a, b) = o.Rcw_f[3 * a + b];
                tf(a) = o.tcw_f[a];
                vf(a) = o.v_f[a];
            }
            pKFi->SetPose(SE3T(Rf, tf));
            const auto Tiw = pKFi->GetPose().template cast<double>();
            corrPoses[pKFi] = Sim3T(Tiw.unit_quaternion(), Tiw.translation(), 1.0);
            if (!pKFi->bImu) continue;
            pKFi->SetVelocity(vf);
            pKFi->SetNewBias(BiasT(o.bias_f[0], o.bias_f[1], o.bias_f[2], o.bias_f[3], o.bias_f[4], o.bias_f[5]));
        }
    if (P) {
        typedef typename std::decay<decltype(B.lLocalMapPoints.front()->GetWorldPos())>::type PosT;
        int p = 0;
        for (const auto& pMP : B.lLocalMapPoints) {                                                      // :4410-4417
            const float* o = pos_out.data() + 3 * (size_t)p++;
            pMP->SetWorldPos(PosT(o[0], o[1], o[2]));
            pMP->UpdateNormalAndDepth();
        }
    }
    pMap->IncreaseChangeIndex();                                                                         // :4419
    return true;
}

}  // namespace msorb_host
}  // namespace ORB_SLAM3

#endif
