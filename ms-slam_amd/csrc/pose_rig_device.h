// The mono edges of Optimizer::PoseOptimization's two-camera arm (src/Optimizer.cc:870-931) and of a one-camera frame whose camera is
// not a pinhole, as the kernel of pose_opt.hip and a host compiler read them (tests/pose_opt_rig_main.cc): GeometricCamera::project /
// projectJac of Pinhole and KannalaBrandt8, EdgeSE3ProjectXYZOnlyPose (the left camera) and EdgeSE3ProjectXYZOnlyPoseToBody (the right
// camera, through mTrl).  Every function restates its reference operator by operator, left to right, in double, without contraction
// (the library and the host program are built with -ffp-contract=off).  Camera parameters are GeometricCamera::mvParameters, floats,
// widened where they are used.
//
// The two float roundings of KannalaBrandt8::project(Vector3d) (KannalaBrandt8.cpp:48-49) are part of the result:
//   * sqrtf is the narrowing of the double square root of the widened argument.  The double root is correctly rounded and carries
//     53 >= 2 * 24 + 2 bits, so the second rounding is innocuous: this IS the correctly rounded sqrtf, on the device and on the host.
//   * atan2f is the narrowing of a double atan2 of the widened arguments, ONCE.  It is not a restatement of glibc's e_atan2f.c (whose
//     answer is within an ulp of the true value but not always the nearest float); tools/atan2f_departure.cc counts how often and by
//     how much the two differ over the (y, x) the projection sees, DESIGN.md holds the figures, and the tests' sensitivity bound D
//     includes theta and psi moved by one float ulp either way.
// A point exactly on the optical axis (x = y = 0) gives KannalaBrandt8::projectJac 0/0 (r2 = 0, :163-169) in the reference; that NaN is
// not restated as a contract: whatever these statements give there is what is summed, and the tests keep away from it.
#pragma once
#include "se3_device.h"

namespace msorb {
namespace rig {

using se3::Pose;

enum { kPinhole = 0, kKannalaBrandt8 = 1 };   // msorb_camera_model.type = GeometricCamera::CAM_PINHOLE / CAM_FISHEYE

struct Camera { int type; float p[8]; };      // msorb_camera_model

SE3_HD float sqrtf_cr(float v) { return (float)sqrt((double)v); }
SE3_HD float atan2f_narrowed(float y, float x) { return (float)atan2((double)y, (double)x); }

// SE3Quat::operator* (se3quat.h:104-110): t = A.t + A.r * B.t, r = A.r * B.r (Eigen's quaternion product), normalizeRotation
SE3_HD Pose compose(const Pose& A, const Pose& B) {
    Pose N;
    double rx, ry, rz;
    se3::rotate(A, B.tx, B.ty, B.tz, rx, ry, rz);
    N.tx = A.tx + rx; N.ty = A.ty + ry; N.tz = A.tz + rz;
    N.qw = ((A.qw * B.qw - A.qx * B.qx) - A.qy * B.qy) - A.qz * B.qz;
    N.qx = ((A.qw * B.qx + A.qx * B.qw) + A.qy * B.qz) - A.qz * B.qy;
    N.qy = ((A.qw * B.qy + A.qy * B.qw) + A.qz * B.qx) - A.qx * B.qz;
    N.qz = ((A.qw * B.qz + A.qz * B.qw) + A.qx * B.qy) - A.qy * B.qx;
    se3::normalize_rotation(N);
    return N;
}

// SE3Quat::map (se3quat.h:217-220): r * xyz + t
SE3_HD void map(const Pose& T, double X, double Y, double Z, double& x, double& y, double& z) {
    se3::rotate(T, X, Y, Z, x, y, z);
    x += T.tx; y += T.ty; z += T.tz;
}

// Eigen's Quaternion::toRotationMatrix
SE3_HD void rotation_matrix(const Pose& T, double (*R)[3]) {
    const double tx = 2 * T.qx, ty = 2 * T.qy, tz = 2 * T.qz;
    const double twx = tx * T.qw, twy = ty * T.qw, twz = tz * T.qw, txx = tx * T.qx, txy = ty * T.qx, txz = tz * T.qx;
    const double tyy = ty * T.qy, tyz = tz * T.qy, tzz = tz * T.qz;
    R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
}

// pCamera->project(Vector3d): Pinhole.cpp:35-41, KannalaBrandt8.cpp:46-65
SE3_HD void project(const Camera& c, double x, double y, double z, double& u, double& v) {
    if (c.type == kPinhole) {
        u = ((double)c.p[0] * x) / z + (double)c.p[2];
        v = ((double)c.p[1] * y) / z + (double)c.p[3];
        return;
    }
    const double x2_plus_y2 = x * x + y * y;
    const double theta = (double)atan2f_narrowed(sqrtf_cr((float)x2_plus_y2), (float)z);
    const double psi = (double)atan2f_narrowed((float)y, (float)x);
    const double theta2 = theta * theta;
    const double theta3 = theta * theta2;
    const double theta5 = theta3 * theta2;
    const double theta7 = theta5 * theta2;
    const double theta9 = theta7 * theta2;
    const double r = (((theta + (double)c.p[4] * theta3) + (double)c.p[5] * theta5) + (double)c.p[6] * theta7) + (double)c.p[7] * theta9;
    u = ((double)c.p[0] * r) * cos(psi) + (double)c.p[2];
    v = ((double)c.p[1] * r) * sin(psi) + (double)c.p[3];
}

// pCamera->projectJac(Vector3d) -> 2 x 3: Pinhole.cpp:71-81, KannalaBrandt8.cpp:145-175 (all double; `3 * mvParameters[4]` and its
// like are int * float, a FLOAT product, widened afterwards)
SE3_HD void project_jac(const Camera& c, double x, double y, double z, double (*Jp)[3]) {
    if (c.type == kPinhole) {
        Jp[0][0] = (double)c.p[0] / z; Jp[0][1] = 0; Jp[0][2] = ((double)-c.p[0] * x) / (z * z);
        Jp[1][0] = 0; Jp[1][1] = (double)c.p[1] / z; Jp[1][2] = ((double)-c.p[1] * y) / (z * z);
        return;
    }
    const double x2 = x * x, y2 = y * y, z2 = z * z;
    const double r2 = x2 + y2;
    const double r = sqrt(r2);
    const double r3 = r2 * r;
    const double theta = atan2(r, z);
    const double theta2 = theta * theta, theta3 = theta2 * theta;
    const double theta4 = theta2 * theta2, theta5 = theta4 * theta;
    const double theta6 = theta2 * theta4, theta7 = theta6 * theta;
    const double theta8 = theta4 * theta4, theta9 = theta8 * theta;
    const double f = (((theta + theta3 * (double)c.p[4]) + theta5 * (double)c.p[5]) + theta7 * (double)c.p[6]) + theta9 * (double)c.p[7];
    const double fd = (((1 + (double)(3 * c.p[4]) * theta2) + (double)(5 * c.p[5]) * theta4) + (double)(7 * c.p[6]) * theta6) +
                      (double)(9 * c.p[7]) * theta8;
    const double fx = (double)c.p[0], fy = (double)c.p[1];
    const double den = r2 * (r2 + z2);
    Jp[0][0] = fx * (((fd * z) * x2) / den + (f * y2) / r3);
    Jp[1][0] = fy * ((((fd * z) * y) * x) / den - ((f * y) * x) / r3);
    Jp[0][1] = fx * ((((fd * z) * y) * x) / den - ((f * y) * x) / r3);
    Jp[1][1] = fy * (((fd * z) * y2) / den + (f * x2) / r3);
    Jp[0][2] = (((double)-c.p[0] * fd) * x) / (r2 + z2);
    Jp[1][2] = (((double)-c.p[1] * fd) * y) / (r2 + z2);
}

// A (2 x 3) * SE3deriv of the point (x, y, z) = [0 z -y 1 0 0; -z 0 x 0 1 0; y -x 0 0 0 1] (OptimizableTypes.cpp:57-60, :101-104):
// the row-by-column sums with the products by the constant zeros left out (they add an exact zero)
SE3_HD void times_se3deriv(const double (*A)[3], double x, double y, double z, double (*J)[6]) {
SE3_UNROLL
    for (int i = 0; i < 2; i++) {   // (unrolled: every index is a constant, the arrays stay in registers)
        J[i][0] = A[i][1] * -z + A[i][2] * y;
        J[i][1] = A[i][0] * z + A[i][2] * -x;
        J[i][2] = A[i][0] * -y + A[i][1] * x;
        J[i][3] = A[i][0]; J[i][4] = A[i][1]; J[i][5] = A[i][2];
    }
}

// The frame's cameras as the edges hold them: mTrl is SE3Quat(q, t), whose constructor normalises (se3quat.h:62-64, Optimizer.cc:923)
struct Rig {
    Camera cam[2];
    Pose Trl;
    double Rrl[3][3];   // mTrl.rotation().toRotationMatrix()
};
SE3_HD void set_trl(Rig& g, const float* q, const float* t) {
    g.Trl = Pose{(double)q[0], (double)q[1], (double)q[2], (double)q[3], (double)t[0], (double)t[1], (double)t[2]};
    se3::normalize_rotation(g.Trl);
    rotation_matrix(g.Trl, g.Rrl);
}

// computeError of both edges (OptimizableTypes.h:41-45, :69-73) -> e[2], chi2() = e . (Omega e) (base_edge.h:60), and the point in
// the LEFT camera's frame, T.map(Xw), which both linearizeOplus start from.  Trw = compose(g.Trl, T), the product the right edge maps
// through: it depends on the pose alone, so the caller forms it once per pose with the same statements.
SE3_HD double edge_error(const Rig& g, const Pose& T, const Pose& Trw, bool right, double ox, double oy, double w, double X, double Y, double Z,
                         double* e, double& x, double& y, double& z) {
    map(T, X, Y, Z, x, y, z);
    double u, v;
    if (right) {
        double xr, yr, zr;
        map(Trw, X, Y, Z, xr, yr, zr);
        project(g.cam[1], xr, yr, zr, u, v);
    } else {
        project(g.cam[0], x, y, z, u, v);
    }
    e[0] = ox - u;
    e[1] = oy - v;
    return e[0] * (w * e[0]) + e[1] * (w * e[1]);
}

// linearizeOplus: left -projectJac(X_l) * SE3deriv (OptimizableTypes.cpp:49-63); right -projectJac(mTrl.map(X_l)) *
// mTrl.rotation().toRotationMatrix() * SE3deriv (:91-107), the products taken left to right.  (x, y, z) = X_l = T.map(Xw).
SE3_HD void edge_jacobian(const Rig& g, bool right, double x, double y, double z, double (*J)[6]) {
    double Jp[2][3], A[2][3];
    if (right) {
        double xr, yr, zr;
        map(g.Trl, x, y, z, xr, yr, zr);
        project_jac(g.cam[1], xr, yr, zr, Jp);
SE3_UNROLL
        for (int i = 0; i < 2; i++)
SE3_UNROLL
            for (int j = 0; j < 3; j++) A[i][j] = (-Jp[i][0] * g.Rrl[0][j] + -Jp[i][1] * g.Rrl[1][j]) + -Jp[i][2] * g.Rrl[2][j];
    } else {
        project_jac(g.cam[0], x, y, z, Jp);
SE3_UNROLL
        for (int i = 0; i < 2; i++)
SE3_UNROLL
            for (int j = 0; j < 3; j++) A[i][j] = -Jp[i][j];
    }
    times_se3deriv(A, x, y, z, J);
}

}  // namespace rig
}  // namespace msorb
