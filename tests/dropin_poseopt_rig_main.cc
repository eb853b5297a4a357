// ms-slam_amd/host/Optimizer_device.h's PoseOptimizationAnyCamera compiled against minimal stand-ins of Frame / MapPoint /
// GeometricCamera / Sophus::SE3f that carry the member names the two-camera arm of Optimizer::PoseOptimization
// (src/Optimizer.cc:870-931) and the camera interface (GetType, CAM_PINHOLE, CAM_FISHEYE, getParameter) use, linked to libmsorb.so.
//
//   dropin_poseopt_rig in.bin out.bin
// in : q[4] t[3] q_rl[4] t_rl[3] (float) | fx fy cx cy mbf (float: the frame's pinhole members) |
//      n_cameras type0 type1 (int) | p0[8] p1[8] (float) | N Nleft nlevels (int) | inv_level_sigma2[nlevels] (float) |
//      N x { x y u_right (float) octave state (int: 0 no point, 1 point, 2 bad point) X Y Z (float) }
//      Entry i is mvKeys[i] for i < Nleft and mvKeysRight[i - Nleft] otherwise when n_cameras == 2; mvKeysUn[i] (and mvKeys[i]) when 1.
// out: ret (int) n_set_pose (int) q[4] t[3] (float) mvbOutlier[N] (uint8), and for a pinhole one-camera frame a second record:
//      the same frame through PoseOptimization (the old path)
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
struct SE3f {
    Quatf q;
    Vec3f t;
    SE3f() {}
    SE3f(const Quatf& q_, const Vec3f& t_) : q(q_), t(t_) {}
    const Quatf& unit_quaternion() const { return q; }
    const Vec3f& translation() const { return t; }
};
struct Point2f { float x, y; };
struct KeyPoint {
    Point2f pt;
    float size, angle, response;
    int octave, class_id;
};
struct GeometricCamera {   // the interface the template reads; neither accessor is const in the reference
    const static unsigned int CAM_PINHOLE = 0;
    const static unsigned int CAM_FISHEYE = 1;
    unsigned int mnType = 0;
    std::vector<float> mvParameters;
    int n_read = 0;
    unsigned int GetType() { return mnType; }
    float getParameter(const int i) { n_read++; return mvParameters[i]; }
};
struct MapPoint {
    static std::mutex mGlobalMutex;
    Vec3f pos;
    bool bad = false;
    bool isBad() const { return bad; }
    Vec3f GetWorldPos() const { return pos; }
};
std::mutex MapPoint::mGlobalMutex;
struct Frame {
    int N = 0, Nleft = -1;
    std::vector<std::shared_ptr<MapPoint>> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<KeyPoint> mvKeys, mvKeysRight, mvKeysUn;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    GeometricCamera* mpCamera = nullptr;
    GeometricCamera* mpCamera2 = nullptr;
    SE3f mTcw, mTrl;
    int n_set_pose = 0;
    SE3f GetPose() const { return mTcw; }
    SE3f GetRelativePoseTrl() { return mTrl; }
    void SetPose(const SE3f& T) { mTcw = T; n_set_pose++; }
};

void dump(FILE* f, int ret, const Frame& F) {
    std::fwrite(&ret, 4, 1, f);
    std::fwrite(&F.n_set_pose, 4, 1, f);
    const float pose[7] = {F.mTcw.q.x(), F.mTcw.q.y(), F.mTcw.q.z(), F.mTcw.q.w(), F.mTcw.t(0), F.mTcw.t(1), F.mTcw.t(2)};
    std::fwrite(pose, 4, 7, f);
    for (int i = 0; i < F.N; i++) { const uint8_t b = F.mvbOutlier[i]; std::fwrite(&b, 1, 1, f); }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    float head[19], par[16];
    int cams[3], dims[3];
    if (std::fread(head, 4, 19, in) != 19 || std::fread(cams, 4, 3, in) != 3 || std::fread(par, 4, 16, in) != 16 || std::fread(dims, 4, 3, in) != 3) return 2;
    Frame F;
    F.mTcw = SE3f(Quatf(head[3], head[0], head[1], head[2]), Vec3f(head[4], head[5], head[6]));
    F.mTrl = SE3f(Quatf(head[10], head[7], head[8], head[9]), Vec3f(head[11], head[12], head[13]));
    F.fx = head[14]; F.fy = head[15]; F.cx = head[16]; F.cy = head[17]; F.mbf = head[18];
    GeometricCamera cam[2];
    for (int c = 0; c < 2; c++) {
        cam[c].mnType = (unsigned)cams[1 + c];
        cam[c].mvParameters.assign(par + 8 * c, par + 8 * c + (cam[c].mnType == GeometricCamera::CAM_PINHOLE ? 4 : 8));
    }
    F.mpCamera = &cam[0];
    if (cams[0] == 2) F.mpCamera2 = &cam[1];
    F.N = dims[0];
    F.Nleft = cams[0] == 2 ? dims[1] : -1;
    F.mvInvLevelSigma2.resize(dims[2]);
    if (std::fread(F.mvInvLevelSigma2.data(), 4, dims[2], in) != (size_t)dims[2]) return 2;
    for (int i = 0; i < F.N; i++) {
        float a[3], X[3];
        int b[2];
        if (std::fread(a, 4, 3, in) != 3 || std::fread(b, 4, 2, in) != 2 || std::fread(X, 4, 3, in) != 3) return 2;
        KeyPoint kp{};
        kp.pt.x = a[0]; kp.pt.y = a[1]; kp.octave = b[0];
        if (F.mpCamera2) {
            (i < F.Nleft ? F.mvKeys : F.mvKeysRight).push_back(kp);
        } else {
            F.mvKeys.push_back(kp);
            F.mvKeysUn.push_back(kp);
        }
        F.mvuRight.push_back(a[2]);
        std::shared_ptr<MapPoint> mp;
        if (b[1]) { mp = std::make_shared<MapPoint>(); mp->pos = Vec3f(X[0], X[1], X[2]); mp->bad = b[1] == 2; }
        F.mvpMapPoints.push_back(mp);
        F.mvbOutlier.push_back(i % 3 == 0);   // stale flags: only the entries with a usable point may change
    }
    std::fclose(in);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    {
        Frame G = F;
        const int ret = ORB_SLAM3::msorb_host::PoseOptimizationAnyCamera(&G);
        dump(out, ret, G);
    }
    if (!F.mpCamera2 && cam[0].mnType == GeometricCamera::CAM_PINHOLE) {
        Frame G = F;
        const int ret = ORB_SLAM3::msorb_host::PoseOptimization(&G);
        dump(out, ret, G);
    }
    std::fclose(out);
    return 0;
}
