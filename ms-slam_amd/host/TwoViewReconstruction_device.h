// TwoViewReconstruction (src/TwoViewReconstruction.cc, include/TwoViewReconstruction.h) on the device entry of libmsorb
// (msorb_two_view_reconstruct), written against the reference's own types by name: a template that compiles inside MS-SLAM, where
// cv::KeyPoint / cv::Point3f / Sophus::SE3f / the Eigen matrices are the real classes, and in tests/dropin_two_view_main.cc, where
// they are minimal stand-ins with the same member names.
//
//   typedef ORB_SLAM3::msorb_host::TwoViewReconstruction<cv::KeyPoint, cv::Point3f, Sophus::SE3f, Eigen::Matrix3f, Eigen::Vector3f>
//       DeviceTwoViewReconstruction;
//
// The constructor (K, sigma = 1.0, iterations = 200) and Reconstruct have the reference's signatures and effects.  Reconstruct builds
// the match list as :52-64 do, draws the minimal sets of all iterations with DUtils::Random::SeedRandOnce(0) / RandomInt and the
// swap-with-back rule of :83-98 (the reference draws them all before its loops too, so rand() is consumed exactly as there:
// 8 * iterations draws), makes ONE device call, and writes T21, vbTriangulated and vP3D where the reference writes them: nothing on
// `return false`, and on the homography branch vP3D is left as it was, because ReconstructH (:725-731) never assigns it.
// GetWinnerPoints() hands out the points of the chosen hypothesis on either branch, for an integrator who repairs that omission.
//
// Fewer than 8 matches: false, without a draw or a call (the reference's draw underflows there; Tracking never calls it below 100).
// The arithmetic is csrc/two_view_device.h: parity with a compiled Eigen is not pinned.
#ifndef MSORB_TWOVIEWRECONSTRUCTION_DEVICE_H
#define MSORB_TWOVIEWRECONSTRUCTION_DEVICE_H

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "msorb.h"

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

template <class KeyPoint, class Point3, class SE3, class Matrix3, class Vector3>
class TwoViewReconstruction {
public:
    typedef std::pair<int, int> Match;

    // :32-39; K as Pinhole::toK_ gives it: fx, fy, cx, cy are read, a skew is not
    template <class MatrixK>
    TwoViewReconstruction(const MatrixK& k, float sigma = 1.0f, int iterations = 200, int device = 0)
        : mfx(k(0, 0)), mfy(k(1, 1)), mcx(k(0, 2)), mcy(k(1, 2)), mSigma(sigma), mMaxIterations(iterations), mDevice(device) {}

    // :41-129
    bool Reconstruct(const std::vector<KeyPoint>& vKeys1, const std::vector<KeyPoint>& vKeys2, const std::vector<int>& vMatches12, SE3& T21,
                     std::vector<Point3>& vP3D, std::vector<bool>& vbTriangulated) {
        mvWinnerPoints.clear();
        mBranch = 0;
        // :52-64
        mvMatches12.clear();
        mvMatches12.reserve(vKeys2.size());
        mvbMatched1.resize(vKeys1.size());
        for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {
            if (vMatches12[i] >= 0) {
                mvMatches12.push_back(std::make_pair((int)i, vMatches12[i]));
                mvbMatched1[i] = true;
            } else {
                mvbMatched1[i] = false;
            }
        }
        const int N = (int)mvMatches12.size();
        if (N < 8 || mMaxIterations < 1) return false;
        // :68-98
        std::vector<size_t> vAllIndices, vAvailableIndices;
        vAllIndices.reserve(N);
        for (int i = 0; i < N; i++) vAllIndices.push_back(i);
        mvSets.assign(8 * (size_t)mMaxIterations, 0);
        DUtils::Random::SeedRandOnce(0);
        for (int it = 0; it < mMaxIterations; it++) {
            vAvailableIndices = vAllIndices;
            for (size_t j = 0; j < 8; j++) {
                const int randi = DUtils::Random::RandomInt(0, (int)vAvailableIndices.size() - 1);
                mvSets[8 * (size_t)it + j] = (int)vAvailableIndices[randi];
                vAvailableIndices[randi] = vAvailableIndices.back();
                vAvailableIndices.pop_back();
            }
        }
        // the one call: FindHomography, FindFundamental, the branch, ReconstructH / ReconstructF
        const int n1 = (int)vKeys1.size(), n2 = (int)vKeys2.size();
        std::vector<float> k1(2 * (size_t)n1), k2(2 * (size_t)n2);
        for (int i = 0; i < n1; i++) { k1[2 * (size_t)i] = vKeys1[i].pt.x; k1[2 * (size_t)i + 1] = vKeys1[i].pt.y; }
        for (int i = 0; i < n2; i++) { k2[2 * (size_t)i] = vKeys2[i].pt.x; k2[2 * (size_t)i + 1] = vKeys2[i].pt.y; }
        std::vector<int> m12(n1, -1);
        for (size_t i = 0; i < vMatches12.size() && i < (size_t)n1; i++) m12[i] = vMatches12[i];
        std::vector<uint8_t> tri(n1 ? n1 : 1), inl(N);
        std::vector<float> p3d(3 * (size_t)(n1 ? n1 : 1));
        msorb_two_view_result r;
        const int rc = msorb_two_view_reconstruct(mDevice, n1, k1.data(), n2, k2.data(), m12.data(), mMaxIterations, mvSets.data(), mfx, mfy, mcx,
                                                  mcy, mSigma, 0.50, 1.0f, 50, &r, tri.data(), p3d.data(), inl.data(), nullptr, nullptr,
                                                  nullptr, nullptr);
        if (rc != MSORB_OK) fail_call("msorb_two_view_reconstruct");
        mResult = r;
        mBranch = r.branch;
        if (!r.ok) return false;
        mvWinnerPoints.resize(n1);
        for (int i = 0; i < n1; i++) mvWinnerPoints[i] = Point3{p3d[3 * (size_t)i], p3d[3 * (size_t)i + 1], p3d[3 * (size_t)i + 2]};
        if (r.branch == 2) vP3D = mvWinnerPoints;   // :530 ...; ReconstructH (:725-731) leaves vP3D alone
        vbTriangulated.assign(n1, false);
        for (int i = 0; i < n1; i++) vbTriangulated[i] = tri[i] != 0;
        Matrix3 R;
        Vector3 t;
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) R(a, b) = r.R[3 * a + b];
            t(a) = r.t[a];
        }
        T21 = SE3(R, t);
        return true;
    }

    // vP3D of the hypothesis Reconstruct handed out, indexed by the keypoint of frame 1, on either branch (empty after `false`)
    const std::vector<Point3>& GetWinnerPoints() const { return mvWinnerPoints; }
    // 1: initialised from the homography, 2: from the fundamental matrix, 0: no model (of the last Reconstruct)
    int GetBranch() const { return mBranch; }
    const msorb_two_view_result& GetResult() const { return mResult; }

private:
    std::vector<Match> mvMatches12;
    std::vector<bool> mvbMatched1;
    std::vector<int> mvSets;
    std::vector<Point3> mvWinnerPoints;
    msorb_two_view_result mResult{};
    int mBranch = 0;
    float mfx, mfy, mcx, mcy, mSigma;
    int mMaxIterations, mDevice;
};

}  // namespace msorb_host
}  // namespace ORB_SLAM3

#endif
