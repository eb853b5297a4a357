// Optimizer::PoseOptimization (src/Optimizer.cc:759-1037) on the device entry of libmsorb (msorb_pose_optimization_batch /
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

#include <cstddef>
#include <cstdint>
#include <mutex>
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

}  // namespace msorb_host
}  // namespace ORB_SLAM3

#endif
