// Device pieces of g2o's SE3Quat and robust kernel that the optimisation kernels share (pose_opt.hip, bundle_adjustment.hip, sim3_opt.hip):
// the pose record, Eigen's quaternion rotation, Quaterniond(Matrix3d), SE3Quat::exp, VertexSE3Expmap::oplus, the Huber kernel and
// the 64-lane shuffle of a double.  Plain double arithmetic in the order written (the library is built with -ffp-contract=off).
// A host compiler reads the same statements (tests/sim3_opt_main.cc): everything but the shuffle is __host__ __device__.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SE3_HD __host__ __device__ inline
#define SE3_UNROLL _Pragma("unroll")
#else
#include <math.h>
#define SE3_HD inline
#define SE3_UNROLL
#endif

namespace msorb {
namespace se3 {

struct Pose { double qx, qy, qz, qw, tx, ty, tz; };

// Eigen::Quaternion * Vector3 (QuaternionBase::_transformVector): uv = 2 vec x v; v + w uv + vec x uv
SE3_HD void rotate(const Pose& T, double X, double Y, double Z, double& x, double& y, double& z) {
    double ux = T.qy * Z - T.qz * Y, uy = T.qz * X - T.qx * Z, uz = T.qx * Y - T.qy * X;
    ux += ux; uy += uy; uz += uz;
    x = (X + T.qw * ux) + (T.qy * uz - T.qz * uy);
    y = (Y + T.qw * uy) + (T.qz * ux - T.qx * uz);
    z = (Z + T.qw * uz) + (T.qx * uy - T.qy * ux);
}

// se3quat.h:280-285
SE3_HD void normalize_rotation(Pose& T) {
    if (T.qw < 0) { T.qx *= -1; T.qy *= -1; T.qz *= -1; T.qw *= -1; }
    const double n = sqrt(((T.qx * T.qx + T.qy * T.qy) + T.qz * T.qz) + T.qw * T.qw);
    T.qx /= n; T.qy /= n; T.qz /= n; T.qw /= n;
}

// Quaterniond(Matrix3d) as Eigen converts a rotation matrix (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl) -> x, y, z, w
SE3_HD void quaternion_of_matrix(const double (*R)[3], double* q) {
    double t = (R[0][0] + R[1][1]) + R[2][2];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[2][1] - R[1][2]) * t;
        q[1] = (R[0][2] - R[2][0]) * t;
        q[2] = (R[1][0] - R[0][1]) * t;
    } else {
        int i = 0;
        if (R[1][1] > R[0][0]) i = 1;
        if (R[2][2] > (i ? R[1][1] : R[0][0])) i = 2;
SE3_UNROLL
        for (int a = 0; a < 3; a++)   // (unrolled: every index below is a constant, the arrays stay in registers)
            if (a == i) {
                const int j = (a + 1) % 3, k = (j + 1) % 3;
                t = sqrt(((R[a][a] - R[j][j]) - R[k][k]) + 1.0);
                q[a] = 0.5 * t;
                t = 0.5 / t;
                q[3] = (R[k][j] - R[j][k]) * t;
                q[j] = (R[j][a] + R[a][j]) * t;
                q[k] = (R[k][a] + R[a][k]) * t;
            }
    }
}

// SE3Quat::exp (se3quat.h:223-257), Quaterniond(R) as Eigen converts a rotation matrix, then SE3Quat's constructor (:62-64)
SE3_HD Pose se3_exp(const double* u) {
    const double ox = u[0], oy = u[1], oz = u[2];
    const double theta = sqrt((ox * ox + oy * oy) + oz * oz);
    const double O[3][3] = {{0, -oz, oy}, {oz, 0, -ox}, {-oy, ox, 0}};
    double O2[3][3], R[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) O2[i][j] = (O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j];
    if (theta < 0.00001) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) { R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j]; V[i][j] = R[i][j]; }
    } else {
        double s, c;
        sincos(theta, &s, &c);
        const double a = s / theta, b = (1 - c) / (theta * theta), d = (theta - s) / ((theta * theta) * theta);   // pow(theta, 3)
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double I = i == j ? 1.0 : 0.0;
                R[i][j] = (I + a * O[i][j]) + b * O2[i][j];
                V[i][j] = (I + b * O[i][j]) + d * O2[i][j];
            }
    }
    Pose E;
    double q[4];   // x, y, z, w
    quaternion_of_matrix(R, q);
    E.qx = q[0]; E.qy = q[1]; E.qz = q[2]; E.qw = q[3];
    E.tx = (V[0][0] * u[3] + V[0][1] * u[4]) + V[0][2] * u[5];
    E.ty = (V[1][0] * u[3] + V[1][1] * u[4]) + V[1][2] * u[5];
    E.tz = (V[2][0] * u[3] + V[2][1] * u[4]) + V[2][2] * u[5];
    normalize_rotation(E);
    return E;
}

// VertexSE3Expmap::oplusImpl (types_six_dof_expmap.h:73-76): exp(update) * estimate, SE3Quat::operator* (se3quat.h:104-110)
SE3_HD Pose oplus(const Pose& T, const double* x) {
    const Pose E = se3_exp(x);
    Pose N;
    double rx, ry, rz;
    rotate(E, T.tx, T.ty, T.tz, rx, ry, rz);
    N.tx = E.tx + rx; N.ty = E.ty + ry; N.tz = E.tz + rz;
    N.qw = ((E.qw * T.qw - E.qx * T.qx) - E.qy * T.qy) - E.qz * T.qz;
    N.qx = ((E.qw * T.qx + E.qx * T.qw) + E.qy * T.qz) - E.qz * T.qy;
    N.qy = ((E.qw * T.qy + E.qy * T.qw) + E.qz * T.qx) - E.qx * T.qz;
    N.qz = ((E.qw * T.qz + E.qz * T.qw) + E.qx * T.qy) - E.qy * T.qx;
    normalize_rotation(N);
    return N;
}

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91); without a kernel rho = chi2, rho' = 1 (sparse_optimizer activeRobustChi2)
SE3_HD void huber(double chi2, double delta, bool robust, double& rho0, double& rho1) {
    rho0 = chi2; rho1 = 1.0;
    if (!robust) return;
    const double dsqr = delta * delta;   // setDelta (robust_kernel_impl.cpp:65-69)
    if (chi2 <= dsqr) return;
    const double s = sqrt(chi2);
    rho0 = (2 * s) * delta - dsqr;
    rho1 = delta / s;
}

#if defined(__HIPCC__)
__device__ inline double shfl_xor_f64(double v, int off) { return __shfl_xor(v, off, 64); }
#endif

}  // namespace se3
}  // namespace msorb
