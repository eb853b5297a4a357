// TEST-ONLY stand-ins for what msorb_host::Sim3Solver (ms-slam_amd/host/Sim3Solver_device.h) needs beyond slam_stub_types.h:
// matrices it can WRITE element by element the way Eigen's are written, M(r, c) = v and v(i) = x.
#pragma once
#include "slam_stub_types.h"

namespace Eigen {
struct Matrix4f {
    float m[16];
    float& operator()(int r, int c) { return m[4 * r + c]; }
    float operator()(int r, int c) const { return m[4 * r + c]; }
};
}  // namespace Eigen

namespace sim3_stub {
struct Matrix3f : Eigen::Matrix3f {
    using Eigen::Matrix3f::operator();
    float& operator()(int r, int c) { return m[3 * r + c]; }
};
struct Vector3f : Eigen::Vector3f {
    using Eigen::Vector3f::operator();
    float& operator()(int i) { return v[i]; }
};
}  // namespace sim3_stub
