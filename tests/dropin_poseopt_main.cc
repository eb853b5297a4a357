// ms-slam_amd/host/Optimizer_device.h compiled against minimal stand-ins of Frame / MapPoint / Pinhole / Sophus::SE3f that carry
// the member names Optimizer::PoseOptimization (src/Optimizer.cc:759-1037) uses, linked to libmsorb.so through the C ABI.
//
//   dropin_poseopt in.bin out.bin
// in : q[4] t[3] fx fy cx cy mbf (float) | N nlevels (int) | inv_level_sigma2[nlevels] (float) |
//      N x { x y u_right (float) octave state (int: 0 no point, 1 point, 2 bad point) X Y Z (float) }
// out: three runs { ret (int) q[4] t[3] (float) mvbOutlier[N] (uint8) }: the flat form, the resident-handle form, and a frame
//      with a second camera (must return -1 with the frame untouched)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
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
struct KeyPoint {   // cv::KeyPoint, 28 bytes
    Point2f pt;
    float size, angle, response;
    int octave, class_id;
};
static_assert(sizeof(KeyPoint) == sizeof(msorb_keypoint), "cv::KeyPoint layout");
struct Pinhole {};
struct MapPoint {
    static std::mutex mGlobalMutex;
    Vec3f pos;
    bool bad = false;
    bool isBad() const { return bad; }
    Vec3f GetWorldPos() const { return pos; }
};
std::mutex MapPoint::mGlobalMutex;
struct Frame {
    int N = 0;
    std::vector<std::shared_ptr<MapPoint>> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<KeyPoint> mvKeysUn;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    Pinhole* mpCamera = nullptr;
    Pinhole* mpCamera2 = nullptr;
    SE3f mTcw;
    int n_set_pose = 0;
    SE3f GetPose() const { return mTcw; }
    void SetPose(const SE3f& T) { mTcw = T; n_set_pose++; }
};

void dump(FILE* f, int ret, const Frame& F) {
    std::fwrite(&ret, 4, 1, f);
    const float pose[7] = {F.mTcw.q.x(), F.mTcw.q.y(), F.mTcw.q.z(), F.mTcw.q.w(), F.mTcw.t(0), F.mTcw.t(1), F.mTcw.t(2)};
    std::fwrite(pose, 4, 7, f);
    for (int i = 0; i < F.N; i++) { const uint8_t b = F.mvbOutlier[i]; std::fwrite(&b, 1, 1, f); }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    float head[12];
    int dims[2];
    if (std::fread(head, 4, 12, in) != 12 || std::fread(dims, 4, 2, in) != 2) return 2;
    Frame F0;
    F0.mTcw = SE3f(Quatf(head[3], head[0], head[1], head[2]), Vec3f(head[4], head[5], head[6]));
    F0.fx = head[7]; F0.fy = head[8]; F0.cx = head[9]; F0.cy = head[10]; F0.mbf = head[11];
    F0.N = dims[0];
    F0.mvInvLevelSigma2.resize(dims[1]);
    if (std::fread(F0.mvInvLevelSigma2.data(), 4, dims[1], in) != (size_t)dims[1]) return 2;
    Pinhole cam;
    F0.mpCamera = &cam;
    for (int i = 0; i < F0.N; i++) {
        float a[3], X[3];
        int b[2];
        if (std::fread(a, 4, 3, in) != 3 || std::fread(b, 4, 2, in) != 2 || std::fread(X, 4, 3, in) != 3) return 2;
        KeyPoint kp{};
        kp.pt.x = a[0]; kp.pt.y = a[1]; kp.octave = b[0];
        F0.mvKeysUn.push_back(kp);
        F0.mvuRight.push_back(a[2]);
        std::shared_ptr<MapPoint> mp;
        if (b[1]) { mp = std::make_shared<MapPoint>(); mp->pos = Vec3f(X[0], X[1], X[2]); mp->bad = b[1] == 2; }
        F0.mvpMapPoints.push_back(mp);
        F0.mvbOutlier.push_back(i % 3 == 0);   // stale flags: only the entries with a usable point may change
    }
    std::fclose(in);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    {   // the reference's signature
        Frame F = F0;
        const int ret = ORB_SLAM3::msorb_host::PoseOptimization(&F);
        dump(out, ret, F);
    }
    {   // the keypoints resident on a handle
        Frame F = F0;
        msorb_frame* h = nullptr;
        if (msorb_frame_create(0, &h) != MSORB_OK) return 3;
        std::vector<uint8_t> desc((size_t)F.N * 32, 0);
        std::vector<float> scale(F.mvInvLevelSigma2.size(), 1.0f);
        for (size_t l = 1; l < scale.size(); l++) scale[l] = scale[l - 1] * 1.2f;
        if (msorb_frame_set(h, reinterpret_cast<const msorb_keypoint*>(F.mvKeysUn.data()), F.N, desc.data(), F.mvuRight.data(), -400.0f, 1700.0f,
                            -400.0f, 800.0f, scale.data(), (int)scale.size()) != MSORB_OK)
            return 3;
        const int ret = ORB_SLAM3::msorb_host::PoseOptimization(&F, h);
        dump(out, ret, F);
        msorb_frame_destroy(h);
    }
    {   // a second camera: not handled, nothing touched
        Frame F = F0;
        F.mpCamera2 = &cam;
        int ret = ORB_SLAM3::msorb_host::PoseOptimization(&F);
        if (F.n_set_pose != 0) ret = -100;
        dump(out, ret, F);
    }
    std::fclose(out);
    return 0;
}
