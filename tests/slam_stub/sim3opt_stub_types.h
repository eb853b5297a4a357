// TEST-ONLY stand-ins for what msorb_host::OptimizeSim3 (ms-slam_amd/host/Optimizer_device.h) needs beyond slam_stub_types.h:
// a minimal g2o::Sim3 over double stand-ins of Eigen's quaternion and vector, a 7x7 matrix that can be zeroed, a camera that
// tells its type (GeometricCamera.h: GetType(), CAM_PINHOLE, CAM_FISHEYE) and a KeyFrame with GetRotation / GetTranslation.
#pragma once
#include "slam_stub_types.h"

namespace Eigen {
struct Quaterniond {
    double qw, qx, qy, qz;
    Quaterniond() : qw(1), qx(0), qy(0), qz(0) {}
    Quaterniond(double w, double x, double y, double z) : qw(w), qx(x), qy(y), qz(z) {}   // Eigen's order
    double x() const { return qx; }
    double y() const { return qy; }
    double z() const { return qz; }
    double w() const { return qw; }
};
struct Vector3d {
    double v[3];
    Vector3d() : v{0, 0, 0} {}
    Vector3d(double x, double y, double z) : v{x, y, z} {}
    double operator[](int i) const { return v[i]; }
    double operator()(int i) const { return v[i]; }
};
struct Matrix7d {
    double m[49];
    void setZero() { for (double& x : m) x = 0; }
};
}  // namespace Eigen

namespace g2o {
struct Sim3 {   // Thirdparty/g2o/g2o/types/sim3.h: r, t, s and their accessors; nothing normalises r
    Eigen::Quaterniond r;
    Eigen::Vector3d t;
    double s = 1;
    Sim3() {}
    Sim3(const Eigen::Quaterniond& r_, const Eigen::Vector3d& t_, double s_) : r(r_), t(t_), s(s_) {}
    const Eigen::Quaterniond& rotation() const { return r; }
    const Eigen::Vector3d& translation() const { return t; }
    const double& scale() const { return s; }
};
}  // namespace g2o

namespace sim3opt_stub {
struct Camera : ORB_SLAM3::GeometricCamera {
    static const unsigned int CAM_PINHOLE = 0, CAM_FISHEYE = 1;
    unsigned int mnType = CAM_PINHOLE;
    unsigned int GetType() { return mnType; }
};
struct KeyFrame : ORB_SLAM3::KeyFrame {
    Camera* mpCamera = nullptr;   // (hides the base's pointer: this one can tell its type)
    Eigen::Matrix3f GetRotation() { return GetPose().rotationMatrix(); }
    Eigen::Vector3f GetTranslation() { return GetPose().translation(); }
};
}  // namespace sim3opt_stub
