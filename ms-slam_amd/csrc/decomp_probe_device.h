// The test hook msorb_debug_decomp: ONE call of one small dense decomposition on one record, for the device (decomp_probe.hip) and
// the host (tests/decomp_probe_main.cc).  Nothing is restated here: every case calls the function of the header the kernels
// include.  DESIGN.md section 23.
//
// A record is in_width(op) doubles in and kDecompOut doubles out; outputs a function does not write are 0.  Float functions take
// doubles that are exactly representable floats and return floats widened; an int is returned as a double.  Matrices row major.
//    0 tv_inverse3                  M[9] f               -> inv[9]
//    1 tv_det3                      M[9] f               -> det
//    2 tv_svd3                      A[9] f               -> U[9] S[3] V[9]
//    3 tv_null_vector_8             A[8][9] f            -> x[9], mismatches      (cooperative: 256 lanes, TvWork)
//    4 tv_null_vector_16            A[16][9] f           -> x[9], mismatches      (cooperative: 256 lanes, TvWork)
//    5 np_null_vector               A[16] f              -> x[4]
//    6 sim3_largest_eigenvector     A[16] f              -> q[4]
//    7 sim3_rotation_of_quaternion  q[4] f               -> R[9]
//    8 mlpnp_rank3                  M[9]                 -> rank
//    9 mlpnp_eig3                   M[9]                 -> E[9]
//   10 mlpnp_solve6                 S[36] g[6]           -> dx[6]
//   11 mlpnp_null_vector_12         W[12][12] symmetric  -> x[12], mismatches     (cooperative: 64 lanes, MlpnpWork)
//   12 mlpnp_null_vector_9          W[9][9] symmetric    -> x[9] 0 0 0, mismatches (cooperative: 64 lanes, MlpnpWork)
//   13 inertial_ldlt                n, A[n][n] (the upper triangle is read), b[n], zeros up to 91 -> ok, x[n]
//                                   (n outside 1..kBorderMax, or not an integer: ok = -1 and nothing is called)
// mismatches: the number of lanes whose x is not, bit for bit, lane 0's (out[9] of ops 3 and 4, out[12] of ops 11 and 12); the
// device counts it, the host (one lane) writes 0.
#pragma once
#include "inertial_device.h"
#include "mlpnp_device.h"
#include "sim3_device.h"
#include "two_view_device.h"

namespace msorb {
namespace decompprobe {

constexpr int kDecompOut = 24, kDecompOps = 14;
constexpr int kDecompTvLanes = 256, kDecompMlpnpLanes = 64;   // the workgroups of two_view_hypotheses_kernel and mlpnp_hypotheses_kernel

// doubles one record of `op` reads
SE3_HD int in_width(int op) {
    switch (op) {
    case 3: return 72;
    case 4: case 11: return 144;
    case 5: case 6: return 16;
    case 7: return 4;
    case 10: return 42;
    case 12: return 81;
    case 13: return 1 + inertial::kBorderMax * inertial::kBorderMax + inertial::kBorderMax;
    default: return 9;
    }
}
// 0: one thread per record; 1: a workgroup sharing a TvWork; 2: a workgroup sharing an MlpnpWork
SE3_HD int cooperative(int op) { return op == 3 || op == 4 ? 1 : op == 11 || op == 12 ? 2 : 0; }
// where the cooperative ops keep the mismatch count
SE3_HD int mismatch_slot(int op) { return cooperative(op) == 1 ? 9 : 12; }

// the one-thread ops
SE3_HD void record(int op, const double* a, double* o) {
    for (int k = 0; k < kDecompOut; k++) o[k] = 0.0;
    float f[16], g[21];
    for (int k = 0; k < 16; k++) f[k] = k < in_width(op) && op < 8 ? (float)a[k] : 0.0f;
    for (int k = 0; k < 21; k++) g[k] = 0.0f;
    switch (op) {
    case 0: tv_inverse3(f, g); for (int k = 0; k < 9; k++) o[k] = (double)g[k]; break;
    case 1: o[0] = (double)tv_det3(f); break;
    case 2: tv_svd3(f, g, g + 9, g + 12); for (int k = 0; k < 21; k++) o[k] = (double)g[k]; break;
    case 5: np_null_vector(f, g); for (int k = 0; k < 4; k++) o[k] = (double)g[k]; break;
    case 6: sim3_largest_eigenvector(f, g); for (int k = 0; k < 4; k++) o[k] = (double)g[k]; break;
    case 7: sim3_rotation_of_quaternion(f, g); for (int k = 0; k < 9; k++) o[k] = (double)g[k]; break;
    case 8: o[0] = (double)mlpnp_rank3(a); break;
    case 9: mlpnp_eig3(a, o); break;
    case 10: {
        double S[6][6];
        for (int k = 0; k < 36; k++) S[k / 6][k % 6] = a[k];
        mlpnp_solve6(S, a + 36, o);
        break;
    }
    case 13: {
        o[0] = -1.0;
        if (!(a[0] >= 1.0 && a[0] <= (double)inertial::kBorderMax)) break;
        const int n = (int)a[0];
        if ((double)n != a[0]) break;
        double Lf[inertial::kBorderMax * inertial::kBorderMax], rinv[inertial::kBorderMax];
        const bool ok = inertial::ldlt_factor(n, a + 1, n, Lf, rinv);
        o[0] = ok ? 1.0 : 0.0;
        if (ok) inertial::ldlt_apply(n, Lf, rinv, a + 1 + n * n, 1, o + 1, 1);
        break;
    }
    default: break;
    }
}

// ops 3 and 4 as two_view_hypotheses_kernel calls tv_null_vector: the lanes fill w.A, synchronise, and every lane gets x[9]
SE3_HD void record_tv(TvWork& w, int lane, int stride, int op, const double* a, float* x) {
    const int rows = op == 3 ? 8 : 16;
    for (int k = lane; k < rows * 9; k += stride) w.A[k / 9][k % 9] = (float)a[k];
    TV_SYNC();
    tv_null_vector(w, lane, stride, rows, x);
}

// ops 11 and 12 as mlpnp_compute_pose calls mlpnp_null_vector: the lanes fill w.W and w.V, synchronise, and every lane gets x[12]
SE3_HD void record_mlpnp(MlpnpWork& w, int lane, int stride, int op, const double* a, double* x) {
    const int nc = op == 11 ? 12 : 9;
    for (int e = lane; e < nc * nc; e += stride) {
        w.W[e / nc][e % nc] = a[e];
        w.V[e / nc][e % nc] = e / nc == e % nc ? 1.0 : 0.0;
    }
    MLPNP_SYNC();
    mlpnp_null_vector(w, lane, stride, nc, x);
}

// one record of any op with one lane (the host)
SE3_HD void record_one_lane(int op, const double* a, double* o) {
    if (cooperative(op) == 0) { record(op, a, o); return; }
    for (int k = 0; k < kDecompOut; k++) o[k] = 0.0;
    if (cooperative(op) == 1) {
        TvWork w;
        float x[9];
        record_tv(w, 0, 1, op, a, x);
        for (int k = 0; k < 9; k++) o[k] = (double)x[k];
    } else {
        MlpnpWork w;
        double x[12];
        record_mlpnp(w, 0, 1, op, a, x);
        for (int k = 0; k < 12; k++) o[k] = x[k];
    }
}

}  // namespace decompprobe
}  // namespace msorb
