// Sim3Solver (src/Sim3Solver.cc, include/Sim3Solver.h) on the device entry of libmsorb (msorb_sim3_ransac_batch), written against
// the reference's own types by name: a template that compiles inside MS-SLAM, where KeyFrame / MapPoint / the Eigen matrices are
// the real classes, and in tests/dropin_sim3_main.cc, where they are minimal stand-ins with the same member names.
//
//   typedef ORB_SLAM3::msorb_host::Sim3Solver<shared_ptr<KeyFrame>, shared_ptr<MapPoint>, Eigen::Matrix4f, Eigen::Matrix3f,
//                                             Eigen::Vector3f> DeviceSim3Solver;
//
// The two constructors, SetRansacParameters, both iterate overloads, find and the four getters have the reference's signatures
// and effects.  What runs where: the constructors' filtering (:35-200) and SetRansacParameters (:202-226) are host code.  The
// first iterate after construction or SetRansacParameters draws the minimal sets of ALL mRansacMaxIts iterations with
// DUtils::Random::RandomInt by the reference's swap-with-back rule (:251-265), evaluates them in ONE device call and keeps the
// inlier counts; that iterate and every later one replays the reference's loop (:246-289 / :319-367) over the cached counts in
// chunks of nIterations, and fetches the transform and the inlier mask of the hypothesis a chunk ends on (from the first call's
// answer when it is that call's winner, which is the converged hypothesis whenever there is one; by a one-hypothesis call
// otherwise).
//
// The one difference to the reference: rand() is consumed 3 * mRansacMaxIts times at the first iterate, where the reference stops
// drawing at convergence.  Given the same draws the results are the reference's (up to the float conventions of
// csrc/sim3_device.h).
//
// Not covered: a camera that is not Pinhole, a KeyFrame with mpCamera2.  supported() is then false, nothing is computed, and
// iterate returns the identity with bNoMore set: the caller keeps the reference's solver for such a pair (the library has no
// CPU fallback).  The same holds below three correspondences, where the reference's draw is undefined.
// The second iterate overload returns an uninitialised matrix in the reference when no hypothesis of the chunk reached
// mnBestInliers (:317, :372); here it is the identity.
#ifndef MSORB_SIM3SOLVER_DEVICE_H
#define MSORB_SIM3SOLVER_DEVICE_H

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "msorb.h"
#include "../csrc/sim3_select.h"

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
// GeometricCamera::GetType() == CAM_PINHOLE; a camera type without GetType (the tests' stand-in, which is a pinhole) counts as one
template <class Camera>
auto Sim3IsPinhole(Camera* pCamera, int) -> decltype(pCamera->GetType(), bool()) { return pCamera->GetType() == Camera::CAM_PINHOLE; }
template <class Camera>
bool Sim3IsPinhole(Camera*, long) { return true; }
}  // namespace detail

template <class KeyFramePtr, class MapPointPtr, class Matrix4, class Matrix3, class Vector3>
class Sim3Solver {
public:
    // :35-120
    Sim3Solver(KeyFramePtr pKF1, KeyFramePtr pKF2, const std::vector<MapPointPtr>& vpMatched12, const bool bFixScale = true,
               std::vector<KeyFramePtr> vpKeyFrameMatchedMP = std::vector<KeyFramePtr>(), int device = 0)
        : mbFixScale(bFixScale), mDevice(device) {
        mN1 = (int)vpMatched12.size();
        if (!Admit(pKF1, pKF2)) return;
        bool bDifferentKFs = true;
        if (vpKeyFrameMatchedMP.empty()) {
            bDifferentKFs = false;
            vpKeyFrameMatchedMP = std::vector<KeyFramePtr>(vpMatched12.size(), pKF2);
        }
        const std::vector<MapPointPtr> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        const auto Rcw1 = pKF1->GetRotation();
        const auto tcw1 = pKF1->GetTranslation();
        const auto Rcw2 = pKF2->GetRotation();
        const auto tcw2 = pKF2->GetTranslation();
        KeyFramePtr pKFm = pKF2;
        for (int i1 = 0; i1 < mN1; i1++) {
            if (!vpMatched12[i1]) continue;
            const MapPointPtr pMP1 = vpKeyFrameMP1[i1];
            const MapPointPtr pMP2 = vpMatched12[i1];
            if (!pMP1) continue;
            if (pMP1->isBad() || pMP2->isBad()) continue;
            if (bDifferentKFs) pKFm = vpKeyFrameMatchedMP[i1];
            const int indexKF1 = std::get<0>(pMP1->GetIndexInKeyFrame(pKF1));
            const int indexKF2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKFm));
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            Push(pKF1, pKFm, indexKF1, indexKF2, pMP1, pMP2, i1, Rcw1, tcw1, Rcw2, tcw2);
        }
        SetRansacParameters();
    }

    // :122-200
    Sim3Solver(KeyFramePtr pKFCurr, KeyFramePtr pKFLoop, const std::vector<KeyFramePtr>& vpMatchedCurrentKeyFrame,
               const std::vector<MapPointPtr>& vpMatchedCurrentMapPoint, const std::vector<KeyFramePtr>& vpMatchedLoopKeyFrame,
               const std::vector<MapPointPtr>& vpMatchedLoopMapPoint, const bool bFixScale = true, int device = 0)
        : mbFixScale(bFixScale), mDevice(device) {
        mN1 = (int)vpMatchedCurrentMapPoint.size();
        if (!Admit(pKFCurr, pKFLoop)) return;
        const auto Rcw1 = pKFCurr->GetRotation();
        const auto tcw1 = pKFCurr->GetTranslation();
        const auto Rcw2 = pKFLoop->GetRotation();
        const auto tcw2 = pKFLoop->GetTranslation();
        for (int i1 = 0; i1 < mN1; i1++) {
            const MapPointPtr pMP1 = vpMatchedCurrentMapPoint[i1];
            const MapPointPtr pMP2 = vpMatchedLoopMapPoint[i1];
            if (!pMP1 || !pMP2) continue;
            if (pMP1->isBad() || pMP2->isBad()) continue;
            const KeyFramePtr pKF1 = vpMatchedCurrentKeyFrame[i1];
            const KeyFramePtr pKF2 = vpMatchedLoopKeyFrame[i1];
            if (!pKF1 || !pKF2) continue;
            if (pKF1->isBad() || pKF2->isBad()) continue;
            const int indexKF1 = std::get<0>(pMP1->GetIndexInKeyFrame(pKF1));
            const int indexKF2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKF2));
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            Push(pKF1, pKF2, indexKF1, indexKF2, pMP1, pMP2, i1, Rcw1, tcw1, Rcw2, tcw2);
        }
        SetRansacParameters();
    }

    // false: a camera that is not Pinhole or a KeyFrame with a second camera; the caller keeps the reference's solver
    bool supported() const { return mbSupported; }

    // :202-226.  Forgets the cached evaluation; mnBestInliers stays, as in the reference.
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        mRansacMaxIts = maxIterations;
        N = (int)mvnIndices1.size();
        const float epsilon = (float)mRansacMinInliers / N;
        int nIterations;
        if (mRansacMinInliers == N) {
            nIterations = 1;
        } else {
            // pow and log in double (:221); a NaN or a value outside int converts the way x86 does it
            const double v = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow((double)epsilon, 3)));
            nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN;
        }
        mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
        mnIterations = 0;
        mbEvaluated = false;
    }

    // :375-379
    Matrix4 find(std::vector<bool>& vbInliers12, int& nInliers) {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }

    // :228-295
    Matrix4 iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        bool bConverge;
        Matrix4 best = Identity();
        const Matrix4 T = Replay(nIterations, bNoMore, vbInliers, nInliers, bConverge, best);
        return bConverge ? T : Identity();
    }

    // :297-373
    Matrix4 iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge) {
        Matrix4 best = Identity();
        const Matrix4 T = Replay(nIterations, bNoMore, vbInliers, nInliers, bConverge, best);
        return bConverge ? T : best;
    }

    Matrix4 GetEstimatedTransformation() { return mBestT12; }
    Matrix3 GetEstimatedRotation() { return mBestRotation; }
    Vector3 GetEstimatedTranslation() { return mBestTranslation; }
    float GetEstimatedScale() { return mBestScale; }

private:
    static Matrix4 Identity() {
        Matrix4 T;
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) T(r, c) = r == c ? 1.0f : 0.0f;
        return T;
    }

    template <class KF>
    bool Admit(const KF& pKF1, const KF& pKF2) {
        mBestT12 = Identity();
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) mBestRotation(r, c) = r == c ? 1.0f : 0.0f;
            mBestTranslation(r) = 0.0f;
        }
        mbSupported = !pKF1->mpCamera2 && !pKF2->mpCamera2 && detail::Sim3IsPinhole(pKF1->mpCamera, 0) &&
                      detail::Sim3IsPinhole(pKF2->mpCamera, 0);
        if (!mbSupported) return false;
        for (int i = 0; i < 4; i++) {   // Pinhole::project reads mvParameters[0..3] (Pinhole.cpp:43-49)
            mProblem.cam1[i] = pKF1->mpCamera->getParameter(i);
            mProblem.cam2[i] = pKF2->mpCamera->getParameter(i);
        }
        return true;
    }

    // :93-113 / :173-193 for one surviving match
    template <class KF, class MP, class Rot, class Vec>
    void Push(const KF& pKF1, const KF& pKF2, int indexKF1, int indexKF2, const MP& pMP1, const MP& pMP2, int i1, const Rot& Rcw1,
              const Vec& tcw1, const Rot& Rcw2, const Vec& tcw2) {
        const auto& kp1 = pKF1->GetKeyUn(indexKF1);
        const auto& kp2 = pKF2->GetKeyUn(indexKF2);
        const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
        const float sigmaSquare2 = pKF2->mvLevelSigma2[kp2.octave];
        // mvnMaxError1 / 2 are vector<size_t> (Sim3Solver.h:85-86): the double product is truncated, and :510 compares the float
        // error with that integer converted to float
        mvnMaxError1.push_back((float)(size_t)(9.210 * sigmaSquare1));
        mvnMaxError2.push_back((float)(size_t)(9.210 * sigmaSquare2));
        mvnIndices1.push_back((size_t)i1);
        const auto X3D1w = pMP1->GetWorldPos();
        const auto X1 = (Rcw1 * X3D1w + tcw1).eval();
        const auto X3D2w = pMP2->GetWorldPos();
        const auto X2 = (Rcw2 * X3D2w + tcw2).eval();
        for (int k = 0; k < 3; k++) { mvX3Dc1.push_back(X1(k)); mvX3Dc2.push_back(X2(k)); }
    }

    void Call(const int* triples, int n_hyp, int min_inliers, int best_in, int* counts, msorb_sim3_result& r, std::vector<uint8_t>& mask) {
        mProblem.n = N;
        mProblem.n_hyp = n_hyp;
        mProblem.fix_scale = mbFixScale;
        mProblem.min_inliers = min_inliers;
        mProblem.best_inliers_in = best_in;
        const int corr_offset[2] = {0, N}, hyp_offset[2] = {0, n_hyp};
        mask.assign((size_t)N, 0);
        if (msorb_sim3_ransac_batch(mDevice, 1, &mProblem, corr_offset, hyp_offset, mvX3Dc1.data(), mvX3Dc2.data(), mvnMaxError1.data(),
                                    mvnMaxError2.data(), triples, mask.data(), counts, &r, nullptr) != MSORB_OK)
            fail_call("msorb_sim3_ransac_batch");
    }

    // the draws of all iterations (:251-265) and their evaluation in one call
    void Evaluate() {
        const int H = mRansacMaxIts;
        mTriples.resize(3 * (size_t)H);
        std::vector<size_t> vAvailableIndices;
        for (int h = 0; h < H; h++) {
            vAvailableIndices.resize((size_t)N);
            for (int i = 0; i < N; i++) vAvailableIndices[i] = (size_t)i;   // mvAllIndices
            for (short i = 0; i < 3; ++i) {
                const int randi = DUtils::Random::RandomInt(0, (int)vAvailableIndices.size() - 1);
                mTriples[3 * (size_t)h + i] = (int)vAvailableIndices[randi];
                vAvailableIndices[randi] = vAvailableIndices.back();
                vAvailableIndices.pop_back();
            }
        }
        mCounts.assign((size_t)H, 0);
        Call(mTriples.data(), H, mRansacMinInliers, mnBestInliers, mCounts.data(), mAll, mAllMask);
        mbEvaluated = true;
    }

    // the loop of :246-289 / :319-367 over the cached counts; `best` receives bestSim3 of the second overload
    Matrix4 Replay(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge, Matrix4& best) {
        bNoMore = false;
        bConverge = false;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = 0;
        if (!mbSupported || N < mRansacMinInliers || N < 3) {
            bNoMore = true;
            return Identity();
        }
        if (!mbEvaluated) Evaluate();
        const int first = mnIterations, m = std::max(0, std::min(nIterations, mRansacMaxIts - mnIterations));
        const msorb::Sim3Selection sel = msorb::sim3_select(mCounts.data() + first, m, mRansacMinInliers, mnBestInliers);
        mnIterations += sel.consumed;
        if (sel.winner >= 0) {   // :346-351 at the last hypothesis of the chunk that reached mnBestInliers
            mnBestInliers = sel.best;
            const int h = first + sel.winner;
            msorb_sim3_result one;
            const msorb_sim3_result* r = &mAll;
            const std::vector<uint8_t>* mask = &mAllMask;
            if (h != mAll.winner) {
                int count = 0;
                Call(mTriples.data() + 3 * (size_t)h, 1, INT_MAX, 0, &count, one, mOneMask);
                r = &one;
                mask = &mOneMask;
            }
            for (int row = 0; row < 4; row++)
                for (int c = 0; c < 4; c++) mBestT12(row, c) = r->T12[4 * row + c];
            for (int row = 0; row < 3; row++) {
                for (int c = 0; c < 3; c++) mBestRotation(row, c) = r->R[3 * row + c];
                mBestTranslation(row) = r->t[row];
            }
            mBestScale = r->s;
            best = mBestT12;
            if (sel.converged) {   // :353-361
                nInliers = sel.best;
                for (int i = 0; i < N; i++)
                    if ((*mask)[i]) vbInliers[mvnIndices1[i]] = true;
                bConverge = true;
                return mBestT12;
            }
        }
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return Identity();
    }

    std::vector<float> mvX3Dc1, mvX3Dc2, mvnMaxError1, mvnMaxError2;
    std::vector<size_t> mvnIndices1;
    int N = 0, mN1 = 0;
    int mnIterations = 0, mnBestInliers = 0;
    Matrix4 mBestT12;
    Matrix3 mBestRotation;
    Vector3 mBestTranslation;
    float mBestScale = 0.0f;
    bool mbFixScale;
    double mRansacProb = 0.99;
    int mRansacMinInliers = 6, mRansacMaxIts = 300;
    // the device side
    int mDevice;
    bool mbSupported = false, mbEvaluated = false;
    msorb_sim3_problem mProblem{};
    std::vector<int> mTriples, mCounts;
    msorb_sim3_result mAll{};          // the first call's answer: the loop's end over all hypotheses
    std::vector<uint8_t> mAllMask, mOneMask;
};

}  // namespace msorb_host
}  // namespace ORB_SLAM3
#endif
