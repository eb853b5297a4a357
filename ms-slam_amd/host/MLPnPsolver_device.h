// MLPnPsolver (src/MLPnPsolver.cpp, include/MLPnPsolver.h) on the device entry of libmsorb (msorb_mlpnp_ransac_batch), written against
// the reference's own types by name: a template that compiles inside MS-SLAM, where Frame / KeyFrame / MapPoint / Eigen::Matrix4f are
// the real classes, and in tests/dropin_mlpnp_main.cc, where they are minimal stand-ins with the same member names.
//
//   typedef ORB_SLAM3::msorb_host::MLPnPsolver<Frame, shared_ptr<KeyFrame>, shared_ptr<MapPoint>, Eigen::Matrix4f> DeviceMLPnPsolver;
//
// The two constructors, SetRansacParameters and iterate have the reference's signatures and effects.  What runs where: the
// constructors' filtering (:55-140) and SetRansacParameters (:268-303) are host code.  The loop of iterate (:158) goes on while
// mnIterations < mRansacMaxIts OR nCurrentIterations < nIterations, so a call that does not return early runs
// max(mRansacMaxIts - mnIterations, nIterations) iterations.  The first iterate draws the minimal sets of that many iterations
// with DUtils::Random::RandomInt by the reference's swap-with-back rule (:171-183), evaluates them in ONE device call and keeps
// the counts and poses; that iterate and every later one replay the loop (:212-263, csrc/mlpnp_select.h) over the cached counts,
// and a call that runs past the cache draws and evaluates what it lacks.  The inlier mask of the hypothesis a call ends on comes
// from the evaluating call's answer when it is that call's winner (the first iterate's always is) and from a one-hypothesis call
// otherwise.  EvaluateFirst does the first evaluation of SEVERAL solvers (the relocalisation candidates of
// Tracking::Relocalization) in one device call.
//
// The one difference to the reference: rand() is consumed for all sets of a call at once, where the reference stops drawing when
// a call returns early.  Given the same draws the results are the reference's (up to the conventions of csrc/mlpnp_device.h,
// DESIGN.md section 14).
//
// Not covered: a camera that is not Pinhole.  supported() is then false, nothing is computed, and iterate returns false with
// bNoMore set: the caller keeps the reference's solver for such a frame (the library has no CPU fallback).
#ifndef MSORB_MLPNPSOLVER_DEVICE_H
#define MSORB_MLPNPSOLVER_DEVICE_H

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "msorb.h"
#include "../csrc/mlpnp_select.h"

#include "Thirdparty/DBoW2/DUtils/Random.h"

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

namespace detail {
// GeometricCamera::GetType() == CAM_PINHOLE.  A camera type that cannot say what it is does not compile.
template <class Camera>
bool MlpnpIsPinhole(Camera* pCamera) { return pCamera->GetType() == Camera::CAM_PINHOLE; }
}  // namespace detail

template <class FrameT, class KeyFramePtr, class MapPointPtr, class Matrix4>
class MLPnPsolver {
public:
    // :55-97
    MLPnPsolver(const FrameT& F, const std::vector<MapPointPtr>& vpMapPointMatches, int device = 0) : mDevice(device) {
        mnMatches = vpMapPointMatches.size();
        Admit(F.mpCamera);
        for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
            const MapPointPtr pMP = vpMapPointMatches[i];
            if (!pMP || pMP->isBad()) continue;
            if (i >= F.mvKeysUn.size()) continue;
            const auto& kp = F.mvKeysUn[i];
            Push(kp.pt.x, kp.pt.y, F.mvLevelSigma2[kp.octave], pMP, i);
        }
        SetRansacParameters();
    }

    // :99-140
    MLPnPsolver(const KeyFramePtr pKF, const std::vector<MapPointPtr>& vpMapPointMatches, int device = 0) : mDevice(device) {
        mnMatches = vpMapPointMatches.size();
        Admit(pKF->mpCamera);
        const auto vKeyPoints = pKF->GetAllKeyUn();
        for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
            const MapPointPtr pMP = vpMapPointMatches[i];
            if (!pMP || pMP->isBad()) continue;
            if (i >= vKeyPoints.size()) continue;
            const auto& kp = vKeyPoints[i];
            Push(kp.pt.x, kp.pt.y, pKF->mvLevelSigma2[kp.octave], pMP, i);
        }
        SetRansacParameters();
    }

    // false: a camera that is not Pinhole; the caller keeps the reference's solver
    bool supported() const { return mbSupported; }

    // :268-303.  Forgets the cached evaluation (the thresholds change); mnIterations and the best stay, as in the reference.
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 6, float epsilon = 0.4,
                             float th2 = 5.991) {
        if (mbHaveBest && mvbBestInliers.empty()) mvbBestInliers = MaskOf(mBestHyp);   // under the thresholds it was counted with
        mBestHyp = -1;
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        mRansacMaxIts = maxIterations;
        mRansacEpsilon = epsilon;
        mRansacMinSet = minSet;
        N = (int)mvSigma2.size();
        int nMinInliers = N * mRansacEpsilon;
        if (nMinInliers < mRansacMinInliers) nMinInliers = mRansacMinInliers;
        if (nMinInliers < minSet) nMinInliers = minSet;
        mRansacMinInliers = nMinInliers;
        if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
        int nIterations;
        if (mRansacMinInliers == N) {
            nIterations = 1;
        } else {
            // pow and log in double (:296; the exponent is 3); a NaN or a value outside int converts the way x86 does it
            const double v = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow(mRansacEpsilon, 3)));
            nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN;
        }
        mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
        mvMaxError.resize(mvSigma2.size());
        for (size_t i = 0; i < mvSigma2.size(); i++) mvMaxError[i] = mvSigma2[i] * th2;
        ForgetCache();
    }

    // :143-266
    bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, Matrix4& Tout) {
        SetIdentity(Tout);
        bNoMore = false;
        vbInliers.clear();
        nInliers = 0;
        if (!mbSupported || N < mRansacMinInliers || mRansacMinSet != 6) {   // (the device solves sets of six)
            bNoMore = true;
            return false;
        }
        const int m = IterationsOfACall(nIterations);
        const int first = mnIterations - mCacheFirst;
        if (first + m > (int)mCounts.size()) {
            MLPnPsolver* self = this;
            EvaluateMore(&self, 1, &m);
        }
        const msorb::MlpnpSelection sel = msorb::mlpnp_select(mCounts.data() + first, m, mRansacMinInliers, mnBestInliers);
        mnIterations += sel.consumed;
        if (sel.best_h >= 0) {   // :215-230
            mnBestInliers = sel.best;
            mBestHyp = first + sel.best_h;
            mbHaveBest = true;
            mBestPose.assign(mPoses.begin() + 12 * (size_t)mBestHyp, mPoses.begin() + 12 * (size_t)mBestHyp + 12);
            mvbBestInliers.clear();   // fetched when a call hands it out
        }
        if (sel.converged) {   // :232-243
            const int h = first + sel.winner;
            const std::vector<uint8_t>& mask = MaskOf(h);
            if (h == mBestHyp && sel.best_h == sel.winner) mvbBestInliers = mask;
            nInliers = mCounts[h];
            Hand(mask, &mPoses[12 * (size_t)h], vbInliers, Tout);
            return true;
        }
        if (mnIterations >= mRansacMaxIts) {   // :248-263
            bNoMore = true;
            if (mnBestInliers >= mRansacMinInliers && mbHaveBest) {
                if (mvbBestInliers.empty()) mvbBestInliers = MaskOf(mBestHyp);
                nInliers = mnBestInliers;
                Hand(mvbBestInliers, mBestPose.data(), vbInliers, Tout);
                return true;
            }
        }
        return false;
    }

    // The first evaluation of several solvers in ONE device call: for every solver that is supported, has enough correspondences and
    // has nothing cached, the sets of the call iterate(nIterations, ...) would run, drawn solver by solver in the order given.
    // The iterate calls that follow replay from the cache.  One call runs on one device: solvers constructed for another device
    // than the first one taken are left out and evaluate at their own first iterate.
    static void EvaluateFirst(const std::vector<MLPnPsolver*>& vpSolvers, int nIterations) {
        std::vector<MLPnPsolver*> todo;
        std::vector<int> its;
        for (MLPnPsolver* pSolver : vpSolvers) {
            if (!pSolver) continue;
            MLPnPsolver& s = *pSolver;
            if (!s.mbSupported || s.N < s.mRansacMinInliers || s.mRansacMinSet != 6 || !s.mCounts.empty()) continue;
            if (!todo.empty() && s.mDevice != todo[0]->mDevice) continue;
            todo.push_back(pSolver);
            its.push_back(s.IterationsOfACall(nIterations));
        }
        if (!todo.empty()) EvaluateMore(todo.data(), (int)todo.size(), its.data());
    }

private:
    static void SetIdentity(Matrix4& T) {
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) T(r, c) = r == c ? 1.0f : 0.0f;
    }

    template <class Camera>
    void Admit(Camera* pCamera) {
        mbSupported = pCamera && detail::MlpnpIsPinhole(pCamera);
        if (!mbSupported) return;
        for (int i = 0; i < 4; i++) mCam[i] = pCamera->getParameter(i);   // Pinhole::project / unproject read mvParameters[0..3]
    }

    template <class MP>
    void Push(float x, float y, float sigma2, const MP& pMP, size_t i) {
        mvP2D.push_back(x);
        mvP2D.push_back(y);
        mvSigma2.push_back(sigma2);
        const auto pos = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) mvP3Dw.push_back(pos(k));
        mvKeyPointIndices.push_back(i);
    }

    void ForgetCache() {
        mCacheFirst = mnIterations;
        mSets.clear();
        mCounts.clear();
        mPoses.clear();
        mMaskHyp = -1;
    }

    // the iterations the loop of :158 runs when nothing returns early
    int IterationsOfACall(int nIterations) const { return std::max(std::max(mRansacMaxIts - mnIterations, nIterations), 0); }

    // :163-183 for one iteration, appended to mSets
    void Draw() {
        std::vector<size_t> vAvailableIndices((size_t)N);
        for (int i = 0; i < N; i++) vAvailableIndices[i] = (size_t)i;   // mvAllIndices
        for (short i = 0; i < 6; ++i) {
            const int randi = DUtils::Random::RandomInt(0, (int)vAvailableIndices.size() - 1);
            mSets.push_back((int)vAvailableIndices[randi]);
            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }

    // For each of the n solvers: the hypotheses it lacks to run its[k] iterations from mnIterations on are drawn, and all of them
    // are evaluated in one call on the device of the first (the callers pass solvers of one device).  Each solver keeps the counts and poses and the mask of its part's winner.
    static void EvaluateMore(MLPnPsolver* const* solvers, int n, const int* its) {
        std::vector<msorb_mlpnp_problem> problems((size_t)n);
        std::vector<int> corr_offset(1, 0), hyp_offset(1, 0), sets, old((size_t)n);
        std::vector<float> p2d, p3d, err;
        for (int k = 0; k < n; k++) {
            MLPnPsolver& s = *solvers[k];
            old[k] = (int)s.mCounts.size();
            const int want = s.mnIterations - s.mCacheFirst + its[k];
            for (int h = old[k]; h < want; h++) s.Draw();
            msorb_mlpnp_problem& p = problems[k];
            p.n = s.N;
            p.n_hyp = want - old[k];
            p.min_inliers = s.mRansacMinInliers;
            p.best_inliers_in = s.mnBestInliers;
            for (int i = 0; i < 4; i++) p.cam[i] = s.mCam[i];
            corr_offset.push_back(corr_offset.back() + p.n);
            hyp_offset.push_back(hyp_offset.back() + p.n_hyp);
            sets.insert(sets.end(), s.mSets.begin() + 6 * (size_t)old[k], s.mSets.end());
            p2d.insert(p2d.end(), s.mvP2D.begin(), s.mvP2D.end());
            p3d.insert(p3d.end(), s.mvP3Dw.begin(), s.mvP3Dw.end());
            err.insert(err.end(), s.mvMaxError.begin(), s.mvMaxError.end());
        }
        std::vector<uint8_t> inl((size_t)corr_offset.back());
        std::vector<int> counts((size_t)hyp_offset.back());
        std::vector<double> poses(12 * (size_t)hyp_offset.back());
        std::vector<msorb_mlpnp_result> res((size_t)n);
        if (msorb_mlpnp_ransac_batch(solvers[0]->mDevice, n, problems.data(), corr_offset.data(), hyp_offset.data(), p2d.data(), p3d.data(),
                                     err.data(), sets.data(), inl.data(), counts.data(), poses.data(), nullptr, res.data(), nullptr) != MSORB_OK)
            fail_call("msorb_mlpnp_ransac_batch");
        for (int k = 0; k < n; k++) {
            MLPnPsolver& s = *solvers[k];
            s.mCounts.insert(s.mCounts.end(), counts.begin() + hyp_offset[k], counts.begin() + hyp_offset[k + 1]);
            s.mPoses.insert(s.mPoses.end(), poses.begin() + 12 * (size_t)hyp_offset[k], poses.begin() + 12 * (size_t)hyp_offset[k + 1]);
            s.mMaskHyp = res[k].winner >= 0 ? old[k] + res[k].winner : -1;
            s.mMask.assign(inl.begin() + corr_offset[k], inl.begin() + corr_offset[k + 1]);
        }
    }

    // mvbInliersi of cached hypothesis h
    const std::vector<uint8_t>& MaskOf(int h) {
        if (h == mMaskHyp) return mMask;
        // one hypothesis under min_inliers = 0 and a carried best of -1: it is the call's winner whatever it counts
        msorb_mlpnp_problem p{};
        p.n = N;
        p.n_hyp = 1;
        p.min_inliers = 0;
        p.best_inliers_in = -1;
        for (int i = 0; i < 4; i++) p.cam[i] = mCam[i];
        const int corr_offset[2] = {0, N}, hyp_offset[2] = {0, 1};
        msorb_mlpnp_result r;
        mMask.assign((size_t)N, 0);
        if (msorb_mlpnp_ransac_batch(mDevice, 1, &p, corr_offset, hyp_offset, mvP2D.data(), mvP3Dw.data(), mvMaxError.data(),
                                     &mSets[6 * (size_t)h], mMask.data(), nullptr, nullptr, nullptr, &r, nullptr) != MSORB_OK)
            fail_call("msorb_mlpnp_ransac_batch");
        mMaskHyp = h;
        return mMask;
    }

    // :234-241 / :253-260: vbInliers by keypoint index, Tout = the pose narrowed to float under an identity's last row
    void Hand(const std::vector<uint8_t>& mask, const double* pose, std::vector<bool>& vbInliers, Matrix4& Tout) const {
        vbInliers = std::vector<bool>(mnMatches, false);
        for (int i = 0; i < N; i++)
            if (mask[i]) vbInliers[mvKeyPointIndices[i]] = true;
        SetIdentity(Tout);
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) Tout(r, c) = (float)pose[3 * r + c];
            Tout(r, 3) = (float)pose[9 + r];
        }
    }

    std::vector<float> mvP2D, mvP3Dw, mvSigma2, mvMaxError;
    std::vector<size_t> mvKeyPointIndices;
    size_t mnMatches = 0;   // mvpMapPointMatches.size()
    int N = 0;
    int mnIterations = 0, mnBestInliers = 0;
    std::vector<uint8_t> mvbBestInliers;
    std::vector<double> mBestPose;   // mRi, mti of the best (mBestTcw is their narrowing)
    bool mbHaveBest = false;
    double mRansacProb = 0.99;
    int mRansacMinInliers = 8, mRansacMaxIts = 300, mRansacMinSet = 6;
    float mRansacEpsilon = 0.4f;
    // the device side
    int mDevice;
    bool mbSupported = false;
    float mCam[4] = {0, 0, 0, 0};
    int mCacheFirst = 0;               // mnIterations of cached hypothesis 0
    std::vector<int> mSets, mCounts;   // per cached hypothesis
    std::vector<double> mPoses;
    int mBestHyp = -1, mMaskHyp = -1;  // cached hypothesis the best belongs to / mMask belongs to
    std::vector<uint8_t> mMask;
};

}  // namespace msorb_host
}  // namespace ORB_SLAM3
#endif
