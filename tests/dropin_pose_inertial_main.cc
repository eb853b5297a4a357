// ms-slam_amd/host/Optimizer_device.h's PoseInertialOptimizationLastKeyFrame / LastFrame compiled against minimal stand-ins of
// Frame / KeyFrame / MapPoint / IMU::Preintegrated / IMU::Bias / IMU::Calib / ConstraintPoseImu that carry the member names
// src/Optimizer.cc:4422-5172 uses, linked to libmsorb.so through the C ABI.
//
//   dropin_pose_inertial in.bin          the scenes of tests/pose_inertial_cases.py's write_dropin_scenes
// Every scene becomes a frame whose keypoints are the scene's observations with a keypoint WITHOUT map point after every second
// one.  Checked per scene, against msorb_pose_inertial_optimization_batch on a problem gathered beside the templates: the return
// value, mvbOutlier where there is a point and untouched where there is none, what SetImuPoseVelocity received, mImuBias, the
// new ConstraintPoseImu (its H byte-equal to H_prior although the constructor changes what it is handed), the old one of the
// previous frame deleted in the LastFrame form, the resident-handle form equal to the flat one, and -1 with nothing touched for
// a second camera, Nleft != -1, a missing preintegration and, in the LastFrame form, a previous frame without mpcpi.
// Prints "ok" last.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "Optimizer_device.h"

namespace {

template <class T, int R, int C>
struct Mat {
    T v[R * C];
    Mat() { for (int i = 0; i < R * C; i++) v[i] = 0; }
    T& operator()(int r, int c) { return v[r * C + c]; }
    const T& operator()(int r, int c) const { return v[r * C + c]; }
    T& operator()(int r) { return v[r]; }
    const T& operator()(int r) const { return v[r]; }
};
typedef Mat<float, 3, 3> Matrix3f;
typedef Mat<float, 3, 1> Vector3f;
typedef Mat<double, 3, 3> Matrix3d;
typedef Mat<double, 3, 1> Vector3d;
typedef Mat<double, 15, 15> Matrix15d;
typedef Mat<float, 15, 15> Matrix15f;

struct SE3f {
    Matrix3f R;
    Vector3f t;
    Matrix3f rotationMatrix() const { return R; }
    Vector3f translation() const { return t; }
};
struct Bias {
    float bax = 0, bay = 0, baz = 0, bwx = 0, bwy = 0, bwz = 0;
    Bias() {}
    Bias(float ax, float ay, float az, float wx, float wy, float wz) : bax(ax), bay(ay), baz(az), bwx(wx), bwy(wy), bwz(wz) {}
};
struct Calib { SE3f mTcb, mTbc; };
struct Preintegrated {
    Matrix3f dR, JRg, JVg, JVa, JPg, JPa;
    Vector3f dV, dP;
    Matrix15f C;
    Bias b;
    float dT = 0;
};
int g_constraints_alive = 0;
struct ConstraintPoseImu {
    Matrix3d Rwb;
    Vector3d twb, vwb, bg, ba;
    Matrix15d H;
    ConstraintPoseImu(const Matrix3d& R, const Vector3d& t, const Vector3d& v, const Vector3d& g, const Vector3d& a, const Matrix15d& H_)
        : Rwb(R), twb(t), vwb(v), bg(g), ba(a), H(H_) {
        for (int i = 0; i < 225; i++) H.v[i] = H.v[i] * (1.0 + 1e-12);   // stands for the clipping the real constructor runs again
        g_constraints_alive++;
    }
    ~ConstraintPoseImu() { g_constraints_alive--; }
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
    Vector3f pos;
    float mTrackDepth = 0;
    bool isBad() const { return true; }   // the routine must not ask
    Vector3f GetWorldPos() const { return pos; }
};
std::mutex MapPoint::mGlobalMutex;
struct KeyFrame {
    Matrix3f Rwb;
    Vector3f twb, v, bg, ba;
    Matrix3f GetImuRotation() { return Rwb; }
    Vector3f GetImuPosition() { return twb; }
    Vector3f GetVelocity() { return v; }
    Vector3f GetGyroBias() { return bg; }
    Vector3f GetAccBias() { return ba; }
};
struct Frame {
    int N = 0, Nleft = -1;
    std::vector<std::shared_ptr<MapPoint>> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    std::vector<float> mvuRight, mvInvLevelSigma2;
    std::vector<KeyPoint> mvKeysUn;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    Pinhole* mpCamera = nullptr;
    Pinhole* mpCamera2 = nullptr;
    SE3f mTcw;
    Matrix3f mRwb;
    Vector3f mtwb, mVw;
    Bias mImuBias;
    Calib mImuCalib;
    std::shared_ptr<Preintegrated> mpImuPreintegrated, mpImuPreintegratedFrame;
    std::shared_ptr<KeyFrame> mpLastKeyFrame;
    Frame* mpPrevFrame = nullptr;
    ConstraintPoseImu* mpcpi = nullptr;
    int n_set = 0;
    SE3f GetPose() const { return mTcw; }
    Matrix3f GetImuRotation() { return mRwb; }
    Vector3f GetImuPosition() const { return mtwb; }
    Vector3f GetVelocity() const { return mVw; }
    void SetImuPoseVelocity(const Matrix3f& R, const Vector3f& t, const Vector3f& v) { mRwb = R; mtwb = t; mVw = v; n_set++; }
};

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
int fail(int scene, const char* what) { std::printf("scene %d: %s\n", scene, what); return 1; }

void put3(const double* s, Matrix3f& M) { for (int i = 0; i < 9; i++) M.v[i] = (float)s[i]; }
void put3(const double* s, Vector3f& v) { for (int i = 0; i < 3; i++) v.v[i] = (float)s[i]; }

void inverse3(const float* C, int ld, double* out) {   // the adjugate over the determinant, as the header documents it
    double m[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) m[3 * r + c] = (double)C[r * ld + c];
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double inv = 1.0 / ((m[0] * c00 + m[1] * c01) + m[2] * c02);
    out[0] = c00 * inv; out[1] = (m[2] * m[7] - m[1] * m[8]) * inv; out[2] = (m[1] * m[5] - m[2] * m[4]) * inv;
    out[3] = c01 * inv; out[4] = (m[0] * m[8] - m[2] * m[6]) * inv; out[5] = (m[2] * m[3] - m[0] * m[5]) * inv;
    out[6] = c02 * inv; out[7] = (m[1] * m[6] - m[0] * m[7]) * inv; out[8] = (m[0] * m[4] - m[1] * m[3]) * inv;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    int n_scenes = 0;
    if (!in || !read_exact(in, &n_scenes, 4)) return 2;
    std::vector<msorb_pose_inertial_problem> Pv(1);
    std::vector<msorb_pose_inertial_result> Rv(1);
    Pinhole cam;
    for (int sidx = 0; sidx < n_scenes; sidx++) {
        msorb_pose_inertial_problem& P = Pv[0];
        if (!read_exact(in, &P, sizeof(P)) || P.n < 0) return 2;
        const size_t n = (size_t)P.n;
        std::vector<float> xy(2 * n), ur(n), inv(n), pos(3 * n), table(8), C15(225);
        std::vector<uint8_t> close(n);
        std::vector<int> octave(n);
        if (!read_exact(in, xy.data(), 8 * n) || !read_exact(in, ur.data(), 4 * n) || !read_exact(in, inv.data(), 4 * n) ||
            !read_exact(in, pos.data(), 12 * n) || !read_exact(in, close.data(), n) || !read_exact(in, octave.data(), 4 * n) ||
            !read_exact(in, table.data(), 32) || !read_exact(in, C15.data(), 900))
            return 2;
        // ---- the reference's objects
        auto pre = std::make_shared<Preintegrated>();
        for (int i = 0; i < 9; i++) {
            pre->dR.v[i] = P.pre.dR[i]; pre->JRg.v[i] = P.pre.JRg[i]; pre->JVg.v[i] = P.pre.JVg[i]; pre->JVa.v[i] = P.pre.JVa[i];
            pre->JPg.v[i] = P.pre.JPg[i]; pre->JPa.v[i] = P.pre.JPa[i];
        }
        for (int i = 0; i < 3; i++) { pre->dV.v[i] = P.pre.dV[i]; pre->dP.v[i] = P.pre.dP[i]; }
        for (int i = 0; i < 225; i++) pre->C.v[i] = C15[i];
        pre->b = Bias(P.pre.bias[0], P.pre.bias[1], P.pre.bias[2], P.pre.bias[3], P.pre.bias[4], P.pre.bias[5]);
        pre->dT = P.pre.dT;
        // in the LastFrame form the random-walk blocks come from the preintegration since the last KeyFrame: another object
        auto preKF = std::make_shared<Preintegrated>(*pre);
        if (P.form == 1)
            for (int i = 0; i < 9; i++) preKF->dR.v[i] = 7.0f;   // (must not be read)
        auto kf = std::make_shared<KeyFrame>();
        Frame prev;
        Frame F0;
        F0.mpCamera = &cam;
        F0.fx = P.fx; F0.fy = P.fy; F0.cx = P.cx; F0.cy = P.cy; F0.mbf = P.mbf;
        put3(P.frame.Rwb, F0.mRwb); put3(P.frame.twb, F0.mtwb); put3(P.frame.v, F0.mVw);
        F0.mImuBias = Bias((float)P.frame.ba[0], (float)P.frame.ba[1], (float)P.frame.ba[2], (float)P.frame.bg[0], (float)P.frame.bg[1],
                           (float)P.frame.bg[2]);
        put3(P.Rcw, F0.mTcw.R); put3(P.tcw, F0.mTcw.t);
        put3(P.Rcb, F0.mImuCalib.mTcb.R); put3(P.tcb, F0.mImuCalib.mTcb.t); put3(P.tbc, F0.mImuCalib.mTbc.t);
        F0.mvInvLevelSigma2 = table;
        if (P.form == 0) {
            put3(P.other.Rwb, kf->Rwb); put3(P.other.twb, kf->twb); put3(P.other.v, kf->v); put3(P.other.bg, kf->bg); put3(P.other.ba, kf->ba);
            F0.mpLastKeyFrame = kf;
            F0.mpImuPreintegrated = pre;
        } else {
            put3(P.other.Rwb, prev.mRwb); put3(P.other.twb, prev.mtwb); put3(P.other.v, prev.mVw);
            prev.mImuBias = Bias((float)P.other.ba[0], (float)P.other.ba[1], (float)P.other.ba[2], (float)P.other.bg[0], (float)P.other.bg[1],
                                 (float)P.other.bg[2]);
            F0.mpPrevFrame = &prev;
            F0.mpImuPreintegratedFrame = pre;
            F0.mpImuPreintegrated = preKF;
        }
        std::vector<int> where(n);   // observation k is keypoint where[k]
        for (size_t k = 0; k < n; k++) {
            KeyPoint kp{};
            kp.pt.x = xy[2 * k]; kp.pt.y = xy[2 * k + 1]; kp.octave = octave[k];
            auto mp = std::make_shared<MapPoint>();
            for (int a = 0; a < 3; a++) mp->pos.v[a] = pos[3 * k + a];
            mp->mTrackDepth = close[k] ? 5.0f : 20.0f;
            where[k] = (int)F0.mvKeysUn.size();
            F0.mvKeysUn.push_back(kp); F0.mvuRight.push_back(ur[k]); F0.mvpMapPoints.push_back(mp);
            if (k % 2 == 1) {   // a keypoint without a map point
                kp.pt.x += 3.0f;
                F0.mvKeysUn.push_back(kp); F0.mvuRight.push_back(-1.0f); F0.mvpMapPoints.push_back(nullptr);
            }
        }
        F0.N = (int)F0.mvKeysUn.size();
        for (int i = 0; i < F0.N; i++) F0.mvbOutlier.push_back(i % 3 == 0);   // stale flags
        // ---- the expected result: the problem gathered here, through the C ABI
        msorb_pose_inertial_problem E = P;
        for (int i = 0; i < 9; i++) E.Rcb[i] = (double)(float)P.Rcb[i];
        for (int i = 0; i < 3; i++) E.tcb[i] = (double)(float)P.tcb[i];
        if (!msorb::inertial::info_from_covariance(C15.data(), 15, E.pre.info)) return fail(sidx, "the covariance has no inverse");
        inverse3(C15.data() + 9 * 15 + 9, 15, E.info_gyro);
        inverse3(C15.data() + 12 * 15 + 12, 15, E.info_acc);
        E.pre.kf_prev = E.pre.kf_cur = 0;
        msorb_pose_inertial_result& R = Rv[0];
        std::vector<uint8_t> flags(n + 1, 0);
        const int off[2] = {0, (int)n};
        if (msorb_pose_inertial_optimization_batch(0, 1, &E, off, xy.data(), ur.data(), inv.data(), pos.data(), close.data(), flags.data(), &R,
                                                   nullptr) != MSORB_OK)
            return fail(sidx, msorb_last_error());
        auto make_prior = [&]() {
            Matrix3d Rp;
            Vector3d tp, vp, gp, ap;
            Matrix15d Hp;
            for (int i = 0; i < 9; i++) Rp.v[i] = P.prior.Rwb[i];
            for (int i = 0; i < 3; i++) { tp.v[i] = P.prior.twb[i]; vp.v[i] = P.prior.v[i]; gp.v[i] = P.prior.bg[i]; ap.v[i] = P.prior.ba[i]; }
            ConstraintPoseImu* c = new ConstraintPoseImu(Rp, tp, vp, gp, ap, Hp);
            for (int i = 0; i < 225; i++) c->H.v[i] = P.H[i];
            return c;
        };
        for (int resident = 0; resident < 2; resident++) {
            Frame F = F0;
            if (P.form == 1) prev.mpcpi = make_prior();
            const int alive = g_constraints_alive;
            msorb_frame* h = nullptr;
            int ret;
            if (resident) {
                if (msorb_frame_create(0, &h) != MSORB_OK) return 3;
                std::vector<uint8_t> desc((size_t)F.N * 32, 0);
                std::vector<float> scale(8, 1.0f);
                for (size_t l = 1; l < scale.size(); l++) scale[l] = scale[l - 1] * 1.2f;
                if (msorb_frame_set(h, reinterpret_cast<const msorb_keypoint*>(F.mvKeysUn.data()), F.N, desc.data(), F.mvuRight.data(), -400.0f,
                                    1700.0f, -400.0f, 800.0f, scale.data(), (int)scale.size()) != MSORB_OK)
                    return 3;
                ret = P.form == 0 ? ORB_SLAM3::msorb_host::PoseInertialOptimizationLastKeyFrame(&F, h, P.rec_init != 0)
                                  : ORB_SLAM3::msorb_host::PoseInertialOptimizationLastFrame(&F, h, P.rec_init != 0);
                msorb_frame_destroy(h);
            } else {
                ret = P.form == 0 ? ORB_SLAM3::msorb_host::PoseInertialOptimizationLastKeyFrame(&F, P.rec_init != 0)
                                  : ORB_SLAM3::msorb_host::PoseInertialOptimizationLastFrame(&F, P.rec_init != 0);
            }
            if (ret != R.n_initial - R.n_bad) return fail(sidx, "the return value");
            std::vector<int> point_of(F.N, -1);
            for (size_t k = 0; k < n; k++) point_of[where[k]] = (int)k;
            for (int i = 0; i < F.N; i++) {
                const bool want = point_of[i] >= 0 ? flags[point_of[i]] != 0 : (i % 3 == 0);
                if (F.mvbOutlier[i] != want) return fail(sidx, "mvbOutlier");
            }
            if (F.n_set != 1 || std::memcmp(F.mRwb.v, R.Rwb_f, 36) || std::memcmp(F.mtwb.v, R.twb_f, 12) || std::memcmp(F.mVw.v, R.v_f, 12))
                return fail(sidx, "SetImuPoseVelocity");
            const Bias& b = F.mImuBias;
            if (b.bax != (float)R.est.ba[0] || b.bay != (float)R.est.ba[1] || b.baz != (float)R.est.ba[2] || b.bwx != (float)R.est.bg[0] ||
                b.bwy != (float)R.est.bg[1] || b.bwz != (float)R.est.bg[2])
                return fail(sidx, "mImuBias");
            const ConstraintPoseImu* c = F.mpcpi;
            if (!c || std::memcmp(c->Rwb.v, R.est.Rwb, 72) || std::memcmp(c->twb.v, R.est.twb, 24) || std::memcmp(c->vwb.v, R.est.v, 24) ||
                std::memcmp(c->bg.v, R.est.bg, 24) || std::memcmp(c->ba.v, R.est.ba, 24))
                return fail(sidx, "the new ConstraintPoseImu's state");
            if (std::memcmp(c->H.v, R.H_prior, 1800)) return fail(sidx, "the new ConstraintPoseImu's H is not H_prior");
            if (P.form == 1 && (prev.mpcpi != nullptr || g_constraints_alive != alive)) return fail(sidx, "the previous frame's mpcpi");
            if (P.form == 0 && g_constraints_alive != alive + 1) return fail(sidx, "one new ConstraintPoseImu");
            delete F.mpcpi;
        }
        // ---- not handled: -1, nothing touched
        for (int which = 0; which < 4; which++) {
            if (which == 3 && P.form == 0) continue;
            Frame F = F0;
            if (P.form == 1) prev.mpcpi = make_prior();
            if (which == 0) F.mpCamera2 = &cam;
            if (which == 1) F.Nleft = 0;
            if (which == 2) { if (P.form == 0) F.mpImuPreintegrated.reset(); else F.mpImuPreintegratedFrame.reset(); }
            if (which == 3) { delete prev.mpcpi; prev.mpcpi = nullptr; }
            ConstraintPoseImu* const before = prev.mpcpi;
            const int ret = P.form == 0 ? ORB_SLAM3::msorb_host::PoseInertialOptimizationLastKeyFrame(&F)
                                        : ORB_SLAM3::msorb_host::PoseInertialOptimizationLastFrame(&F);
            if (ret != -1 || F.n_set != 0 || F.mpcpi != nullptr || F.mvbOutlier != F0.mvbOutlier || prev.mpcpi != before)
                return fail(sidx, "a frame that is not handled was touched");
            delete prev.mpcpi;
            prev.mpcpi = nullptr;
        }
        if (g_constraints_alive != 0) return fail(sidx, "a ConstraintPoseImu leaked");
        std::printf("scene %d: form %d n %d N %d -> %d inliers\n", sidx, P.form, P.n, F0.N, R.n_initial - R.n_bad);
    }
    std::fclose(in);
    std::printf("ok\n");
    return 0;
}
