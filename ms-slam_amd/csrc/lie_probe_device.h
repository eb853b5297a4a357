// The test hook msorb_debug_lie: ONE call of one shared Lie-group primitive on one record, for the device (lie_probe.hip) and the
// host (tests/lie_probe_main.cc).  Nothing is restated here: every case calls the function of the header the optimisers include.
// DESIGN.md section 21.
//
// A record is kLieIn doubles in and kLieOut doubles out; outputs a function does not write are 0.  Float functions take doubles
// that are exactly representable floats and return floats widened.  Layouts (in -> out), quaternions as x, y, z, w, matrices row major:
//    0 rotate                       q[4] v[3]            -> v'[3]
//    1 normalize_rotation (se3)     q[4]                 -> q[4]
//    2 quaternion_of_matrix         R[9]                 -> q[4]
//    3 se3_exp                      omega[3] upsilon[3]  -> q[4] t[3]
//    4 oplus                        q[4] t[3] x[6]       -> q[4] t[3]
//    5 huber                        chi2 delta robust    -> rho0 rho1
//    6 sim3_exp                     omega[3] upsilon[3] sigma -> q[4] t[3] s
//    7 sim3_mul                     a: q[4] t[3] s, b: q[4] t[3] s -> q[4] t[3] s
//    8 sim3_inverse                 q[4] t[3] s          -> q[4] t[3] s
//    9 lu3_solve                    W[9] t[3]            -> x[3]
//   10 sim3_log                     q[4] t[3] s          -> omega[3] upsilon[3] sigma
//   11 normalize_rotation (eg4)     T[9]                 -> R[9]
//   12 exp_so3                      w[3]                 -> R[9]
//   13 log_so3                      R[9]                 -> w[3]
//   14 normalize_rotation_f         T[9] (floats)        -> R[9]
//   15 so3f_exp_matrix              w[3] (floats)        -> R[9]
//   16 bias_corrected               FIVE consecutive records, 80 doubles: dR[9] dV[3] dP[3] JRg[9] JVg[9] JVa[9] JPg[9] JPa[9]
//                                   bias[6] (all floats: the fields of msorb_inertial_edge the function reads, nothing else of
//                                   the edge is filled), then the doubles bg[3] ba[3], 8 unused -> dR[9] dV[3] dP[3] dbg[3]
//   17 right_jacobian_so3           w[3]                 -> J[9]
//   18 inverse_right_jacobian_so3   w[3]                 -> J[9]
//   19 mlpnp_nearest_rotation       T[9]                 -> R[9]
//   20 mlpnp_rodrigues2rot          w[3]                 -> R[9]
//   21 mlpnp_rot2rodrigues          R[9]                 -> w[3]
#pragma once
#include "essential_graph_device.h"
#include "inertial_device.h"
#include "mlpnp_device.h"

namespace msorb {
namespace lieprobe {

constexpr int kLieIn = 16, kLieOut = 24, kLieOps = 22;

// input records one call of `op` reads
SE3_HD int in_records(int op) { return op == 16 ? 5 : 1; }

SE3_HD void put_pose(const se3::Pose& T, double* o) {
    o[0] = T.qx; o[1] = T.qy; o[2] = T.qz; o[3] = T.qw; o[4] = T.tx; o[5] = T.ty; o[6] = T.tz;
}
SE3_HD sim3opt::Sim3 get_sim3(const double* a) { return sim3opt::Sim3{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]}; }
SE3_HD void put_sim3(const sim3opt::Sim3& S, double* o) {
    o[0] = S.qx; o[1] = S.qy; o[2] = S.qz; o[3] = S.qw; o[4] = S.tx; o[5] = S.ty; o[6] = S.tz; o[7] = S.s;
}

SE3_HD void record(int op, const double* a, double* o) {
    for (int k = 0; k < kLieOut; k++) o[k] = 0.0;
    switch (op) {
    case 0: {
        const se3::Pose T{a[0], a[1], a[2], a[3], 0, 0, 0};
        se3::rotate(T, a[4], a[5], a[6], o[0], o[1], o[2]);
        break;
    }
    case 1: {
        se3::Pose T{a[0], a[1], a[2], a[3], 0, 0, 0};
        se3::normalize_rotation(T);
        o[0] = T.qx; o[1] = T.qy; o[2] = T.qz; o[3] = T.qw;
        break;
    }
    case 2: {
        const double R[3][3] = {{a[0], a[1], a[2]}, {a[3], a[4], a[5]}, {a[6], a[7], a[8]}};
        se3::quaternion_of_matrix(R, o);
        break;
    }
    case 3: put_pose(se3::se3_exp(a), o); break;
    case 4: {
        const se3::Pose T{a[0], a[1], a[2], a[3], a[4], a[5], a[6]};
        put_pose(se3::oplus(T, a + 7), o);
        break;
    }
    case 5: se3::huber(a[0], a[1], a[2] != 0.0, o[0], o[1]); break;
    case 6: put_sim3(sim3opt::sim3_exp(a), o); break;
    case 7: put_sim3(sim3opt::sim3_mul(get_sim3(a), get_sim3(a + 8)), o); break;
    case 8: put_sim3(sim3opt::sim3_inverse(get_sim3(a)), o); break;
    case 9: {
        double W[3][3] = {{a[0], a[1], a[2]}, {a[3], a[4], a[5]}, {a[6], a[7], a[8]}};
        eg::lu3_solve(W, a + 9, o);
        break;
    }
    case 10: eg::sim3_log(get_sim3(a), o); break;
    case 11: eg4::normalize_rotation(a, o); break;
    case 12: eg4::exp_so3(a[0], a[1], a[2], o); break;
    case 13: eg4::log_so3(a, o); break;
    case 14: case 15: {
        float x[9], y[9];
        for (int k = 0; k < 9; k++) x[k] = (float)a[k];
        if (op == 14) inertial::normalize_rotation_f(x, y);
        else inertial::so3f_exp_matrix(x, y);
        for (int k = 0; k < 9; k++) o[k] = (double)y[k];
        break;
    }
    case 16: {
        msorb_inertial_edge E;
        inertial::Globals G;
        for (int k = 0; k < 9; k++) {
            E.dR[k] = (float)a[k]; E.JRg[k] = (float)a[15 + k]; E.JVg[k] = (float)a[24 + k]; E.JVa[k] = (float)a[33 + k];
            E.JPg[k] = (float)a[42 + k]; E.JPa[k] = (float)a[51 + k];
        }
        for (int k = 0; k < 3; k++) { E.dV[k] = (float)a[9 + k]; E.dP[k] = (float)a[12 + k]; G.bg[k] = a[66 + k]; G.ba[k] = a[69 + k]; }
        for (int k = 0; k < 6; k++) E.bias[k] = (float)a[60 + k];
        inertial::bias_corrected(E, G, o, o + 9, o + 12, o + 15);
        break;
    }
    case 17: inertial::right_jacobian_so3(a[0], a[1], a[2], o); break;
    case 18: inertial::inverse_right_jacobian_so3(a[0], a[1], a[2], o); break;
    case 19: mlpnp_nearest_rotation(a, o); break;
    case 20: mlpnp_rodrigues2rot(a, o); break;
    case 21: mlpnp_rot2rodrigues(a, o); break;
    default: break;
    }
}

}  // namespace lieprobe
}  // namespace msorb
