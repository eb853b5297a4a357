// The kernels under the engine of msorb_local_ba, msorb_bundle_adjustment and msorb_welding_ba (bundle_adjustment.hip): the edge
// linearisation with the Huber switch, the per-vertex gathers, the point inverse, the Schur complement over the plan's index lists,
// the update, the cost / scale reduction, the welding entry's classification, and the stage timer.  bundle_adjustment.hip's header
// comment and DESIGN.md sections 10, 16 and 27 say what each does.  Every sum walks an index list of local_ba_plan.h in a fixed order: no floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/msorb.h"
#include "hip_host.h"
#include "se3_device.h"

namespace msorb {
namespace ba {

using namespace msorb::se3;

constexpr int kEdgeThreads = 256;
// planes of the edge-major linearisation
constexpr int kHll = 0, kBl = 6, kHpp = 9, kBp = 30, kW = 36, kPlanes = 54;

struct BaRes {
    double chi, scale, max_diag;
    int solver_ok, pad;
};

struct BaDev {
    int K, Kf, P, E, n, n_pairs, n_blocks;
    const msorb_ba_keyframe* kf;
    const int *free_of_kf, *kf_of_free, *edge_kf, *edge_pt, *point_begin, *kf_begin, *kf_edge, *pair_begin, *pair_i, *pair_j, *pair_a, *pair_b;
    const float *xy, *ur, *w;
    double *pose[2], *pt[2];   // the two copies of the state: 7 per KeyFrame (q x y z w, t), 3 per point
    double *lin, *Hpp, *Hll, *Dinv, *S, *bs, *x, *part_cost, *part_vtx;
    BaRes* res;
    uint8_t* outlier;
    float d_mono, d_stereo;    // (float)sqrt(5.991), (float)sqrt(7.815): Optimizer.cc:1190-1191
    int robust;                // 0: no robust kernel, rho = chi2 and weight 1 (BundleAdjustment's bRobust, Optimizer.cc:174, :206)
};

struct EdgeGeom {
    double e[3], x, y, z, chi2;
    bool stereo;
};

__device__ inline Pose load_pose(const double* p) { return Pose{p[0], p[1], p[2], p[3], p[4], p[5], p[6]}; }

// computeError of the two binary edges and chi2() = e . (Omega e) (base_edge.h:60).  Stereo: types_six_dof_expmap.h with
// cam_project (types_six_dof_expmap.cpp:190-196, whose invz is a FLOAT); mono: obs - Pinhole::project(map(Xw)).
__device__ inline EdgeGeom edge_geom(const BaDev& A, int s, int e, int& k, int& p) {
    k = A.edge_kf[e];
    p = A.edge_pt[e];
    const Pose T = load_pose(A.pose[s] + 7 * (size_t)k);
    const double* X = A.pt[s] + 3 * (size_t)p;
    const msorb_ba_keyframe c = A.kf[k];
    EdgeGeom g;
    rotate(T, X[0], X[1], X[2], g.x, g.y, g.z);
    g.x += T.tx; g.y += T.ty; g.z += T.tz;
    const double ox = (double)A.xy[2 * (size_t)e], oy = (double)A.xy[2 * (size_t)e + 1], w = (double)A.w[e];
    const float ur = A.ur[e];
    g.stereo = ur >= 0;   // :1246
    const double fx = (double)c.fx, fy = (double)c.fy, cx = (double)c.cx, cy = (double)c.cy;
    if (g.stereo) {
        const double invz = (double)(float)(1.0 / g.z);
        const double p0 = (g.x * invz) * fx + cx;
        g.e[0] = ox - p0;
        g.e[1] = oy - ((g.y * invz) * fy + cy);
        g.e[2] = (double)ur - (p0 - (double)c.mbf * invz);
        g.chi2 = (g.e[0] * (w * g.e[0]) + g.e[1] * (w * g.e[1])) + g.e[2] * (w * g.e[2]);
    } else {
        g.e[0] = ox - ((fx * g.x) / g.z + cx);
        g.e[1] = oy - ((fy * g.y) / g.z + cy);
        g.e[2] = 0;
        g.chi2 = g.e[0] * (w * g.e[0]) + g.e[1] * (w * g.e[1]);
    }
    return g;
}

// sums v over the workgroup (kEdgeThreads threads); thread 0 returns the total: lanes by xor butterfly, then the wavefronts ascending
__device__ inline double block_sum_256(double v, double* lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += shfl_xor_f64(v, off);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = lds[0];
    for (int w = 1; w < kEdgeThreads / 64; w++) s += lds[w];
    return s;
}

// FULL: computeActiveErrors + activeRobustChi2 + buildSystem (levenberg.cpp:75-87).  !FULL: the first two (levenberg.cpp:123-124).
template <bool FULL>
__global__ __launch_bounds__(kEdgeThreads) void ba_edges_kernel(const BaDev A, int s) {
    __shared__ double lds[kEdgeThreads / 64];
    const int e = blockIdx.x * kEdgeThreads + threadIdx.x;
    double rho0 = 0;
    if (e < A.E) {
        int k, p;
        const EdgeGeom g = edge_geom(A, s, e, k, p);
        double rho1;
        huber(g.chi2, (double)(g.stereo ? A.d_stereo : A.d_mono), A.robust != 0, rho0, rho1);
        if constexpr (FULL) {
            const size_t E = (size_t)A.E;
            double* L = A.lin + e;
            const msorb_ba_keyframe c = A.kf[k];
            const double fx = (double)c.fx, fy = (double)c.fy, bf = (double)c.mbf;
            const double x = g.x, y = g.y, z = g.z;
            const int D = g.stereo ? 3 : 2;
            const double w = (double)A.w[e], wr = rho1 * w;   // robustInformation (base_edge.h:96-100)
            double omr[3];                                    // omega_r = -Omega e, times rho' (base_binary_edge.hpp:74,99)
            for (int d = 0; d < 3; d++) omr[d] = (-(w * g.e[d])) * rho1;
            // Eigen's Quaternion::toRotationMatrix
            const Pose T = load_pose(A.pose[s] + 7 * (size_t)k);
            double R[3][3];
            {
                const double tx = 2 * T.qx, ty = 2 * T.qy, tz = 2 * T.qz;
                const double twx = tx * T.qw, twy = ty * T.qw, twz = tz * T.qw, txx = tx * T.qx, txy = ty * T.qx, txz = tz * T.qx;
                const double tyy = ty * T.qy, tyz = tz * T.qy, tzz = tz * T.qz;
                R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
                R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
                R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
            }
            double Ja[3][3], Jb[3][6];   // _jacobianOplusXi (point), _jacobianOplusXj (pose)
            if (g.stereo) {              // types_six_dof_expmap.cpp:228-274
                const double z_2 = z * z;
                for (int j = 0; j < 3; j++) {
                    Ja[0][j] = (-fx * R[0][j]) / z + ((fx * x) * R[2][j]) / z_2;
                    Ja[1][j] = (-fy * R[1][j]) / z + ((fy * y) * R[2][j]) / z_2;
                    Ja[2][j] = Ja[0][j] - (bf * R[2][j]) / z_2;
                }
                Jb[0][0] = ((x * y) / z_2) * fx;
                Jb[0][1] = -(1 + ((x * x) / z_2)) * fx;
                Jb[0][2] = (y / z) * fx;
                Jb[0][3] = (-1. / z) * fx;
                Jb[0][4] = 0;
                Jb[0][5] = (x / z_2) * fx;
                Jb[1][0] = (1 + (y * y) / z_2) * fy;
                Jb[1][1] = ((-x * y) / z_2) * fy;
                Jb[1][2] = (-x / z) * fy;
                Jb[1][3] = 0;
                Jb[1][4] = (-1. / z) * fy;
                Jb[1][5] = (y / z_2) * fy;
                Jb[2][0] = Jb[0][0] - (bf * y) / z_2;
                Jb[2][1] = Jb[0][1] + (bf * x) / z_2;
                Jb[2][2] = Jb[0][2];
                Jb[2][3] = Jb[0][3];
                Jb[2][4] = 0;
                Jb[2][5] = Jb[0][5] - bf / z_2;
            } else {                     // OptimizableTypes.cpp:139-160 with Pinhole::projectJac (Pinhole.cpp:71-81)
                const double a = fx / z, gg = (-fx * x) / (z * z), b = fy / z, d = (-fy * y) / (z * z);
                for (int j = 0; j < 3; j++) {   // -projectJac * R (the products with projectJac's zeros left out)
                    Ja[0][j] = (-a) * R[0][j] + (-gg) * R[2][j];
                    Ja[1][j] = (-b) * R[1][j] + (-d) * R[2][j];
                    Ja[2][j] = 0;
                }
                Jb[0][0] = -(gg * y);          Jb[0][1] = -(a * z + gg * -x); Jb[0][2] = -(a * -y); Jb[0][3] = -a; Jb[0][4] = 0;  Jb[0][5] = -gg;
                Jb[1][0] = -(b * -z + d * y);  Jb[1][1] = -(d * -x);          Jb[1][2] = -(b * x);  Jb[1][3] = 0;  Jb[1][4] = -b; Jb[1][5] = -d;
                for (int j = 0; j < 6; j++) Jb[2][j] = 0;
            }
            // constructQuadraticForm (base_binary_edge.hpp:99-113); a product of small matrices is the plain sum, left to right
            auto quad = [&](const double* ua, int sa, const double* ub, int sb) {   // sum_d (ua[d] wr) ub[d]
                double t = (ua[0] * wr) * ub[0] + (ua[sa] * wr) * ub[sb];
                if (D == 3) t += (ua[2 * sa] * wr) * ub[2 * sb];
                return t;
            };
            auto dotr = [&](const double* ua, int sa) {                              // sum_d ua[d] omr[d]
                double t = ua[0] * omr[0] + ua[sa] * omr[1];
                if (D == 3) t += ua[2 * sa] * omr[2];
                return t;
            };
            int q = kHll;
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = a; b < 3; b++) L[(size_t)(q++) * E] = quad(&Ja[0][a], 3, &Ja[0][b], 3);
#pragma unroll
            for (int a = 0; a < 3; a++) L[(size_t)(kBl + a) * E] = dotr(&Ja[0][a], 3);
            if (A.free_of_kf[k] >= 0) {   // no pose Jacobian, no Hpp, no Hpl for a fixed KeyFrame (:65-66)
                q = kHpp;
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = a; b < 6; b++) L[(size_t)(q++) * E] = quad(&Jb[0][a], 6, &Jb[0][b], 6);
#pragma unroll
                for (int a = 0; a < 6; a++) L[(size_t)(kBp + a) * E] = dotr(&Jb[0][a], 6);
#pragma unroll
                for (int a = 0; a < 6; a++)
#pragma unroll
                    for (int b = 0; b < 3; b++) L[(size_t)(kW + 3 * a + b) * E] = quad(&Jb[0][a], 6, &Ja[0][b], 3);
            }
        }
    }
    const double total = block_sum_256(rho0, lds);
    if (threadIdx.x == 0) A.part_cost[blockIdx.x] = total;
}

// blocks [0, ceil(P / 256)): one thread per point; blocks after them: one wavefront per free KeyFrame
static __global__ __launch_bounds__(kEdgeThreads) void ba_gather_kernel(const BaDev A, int point_blocks) {
    const size_t E = (size_t)A.E;
    if ((int)blockIdx.x < point_blocks) {
        const int p = blockIdx.x * kEdgeThreads + threadIdx.x;
        if (p >= A.P) return;
        double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int e = A.point_begin[p]; e < A.point_begin[p + 1]; e++)
#pragma unroll
            for (int q = 0; q < 9; q++) S[q] += A.lin[(size_t)q * E + e];
#pragma unroll
        for (int q = 0; q < 9; q++) A.Hll[9 * (size_t)p + q] = S[q];
        A.part_vtx[A.Kf + p] = fmax(fmax(fabs(S[0]), fabs(S[3])), fabs(S[5]));   // computeLambdaInit's share (levenberg.cpp:177-184)
        return;
    }
    const int i = ((int)blockIdx.x - point_blocks) * (kEdgeThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= A.Kf) return;
    double S[27];
#pragma unroll
    for (int q = 0; q < 27; q++) S[q] = 0;
    for (int m = A.kf_begin[i] + lane; m < A.kf_begin[i + 1]; m += 64) {
        const int e = A.kf_edge[m];
#pragma unroll
        for (int q = 0; q < 27; q++) S[q] += A.lin[(size_t)(kHpp + q) * E + e];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int q = 0; q < 27; q++) S[q] += shfl_xor_f64(S[q], off);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 27; q++) A.Hpp[27 * (size_t)i + q] = S[q];
        double m = 0;
        m = fmax(fabs(S[0]), m); m = fmax(fabs(S[6]), m); m = fmax(fabs(S[11]), m);
        m = fmax(fabs(S[15]), m); m = fmax(fabs(S[18]), m); m = fmax(fabs(S[20]), m);
        A.part_vtx[i] = m;
    }
}

// one workgroup: res->chi = the sum of the cost partials; vtx 1: res->max_diag = max of part_vtx; vtx 2: res->scale = its sum
// (computeScale, levenberg.cpp:188-195: KeyFrames first, then points)
static __global__ __launch_bounds__(kEdgeThreads) void ba_finalize_kernel(const BaDev A, int vtx) {
    __shared__ double lds[kEdgeThreads / 64];
    double c = 0;
    for (int i = threadIdx.x; i < A.n_blocks; i += kEdgeThreads) c += A.part_cost[i];
    c = block_sum_256(c, lds);
    if (threadIdx.x == 0) A.res->chi = c;
    const int nv = A.Kf + A.P;
    if (vtx == 1) {
        double m = 0;
        for (int i = threadIdx.x; i < nv; i += kEdgeThreads) m = fmax(A.part_vtx[i], m);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmax(m, shfl_xor_f64(m, off));
        __syncthreads();
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) A.res->max_diag = fmax(fmax(lds[0], lds[1]), fmax(lds[2], lds[3]));
    } else if (vtx == 2) {
        double v = 0;
        for (int i = threadIdx.x; i < nv; i += kEdgeThreads) v += A.part_vtx[i];
        __syncthreads();
        v = block_sum_256(v, lds);
        if (threadIdx.x == 0) A.res->scale = v;
    }
}

// Dinv = D->inverse() (block_solver.hpp:389) as Eigen computes a 3x3 inverse: cofactors times 1 / det, det along the first
// column; D = Hll + lambda I read from its upper triangle.  Then db = Dinv bl (:391-395).  -> Dinv[p]: 6 (upper) + 3
static __global__ __launch_bounds__(kEdgeThreads) void ba_point_inverse_kernel(const BaDev A, double lambda) {
    const int p = blockIdx.x * kEdgeThreads + threadIdx.x;
    if (p >= A.P) return;
    const double* H = A.Hll + 9 * (size_t)p;
    const double m00 = H[0] + lambda, m01 = H[1], m02 = H[2], m11 = H[3] + lambda, m12 = H[4], m22 = H[5] + lambda;
    const double c00 = m11 * m22 - m12 * m12, c10 = m12 * m02 - m22 * m01, c20 = m01 * m12 - m02 * m11;
    const double det = (c00 * m00 + c10 * m01) + c20 * m02, inv = 1.0 / det;
    const double i00 = c00 * inv, i01 = c10 * inv, i02 = c20 * inv;
    const double i11 = (m22 * m00 - m02 * m02) * inv, i12 = (m02 * m01 - m00 * m12) * inv, i22 = (m00 * m11 - m01 * m01) * inv;
    double* o = A.Dinv + 9 * (size_t)p;
    o[0] = i00; o[1] = i01; o[2] = i02; o[3] = i11; o[4] = i12; o[5] = i22;
    o[6] = (i00 * H[6] + i01 * H[7]) + i02 * H[8];
    o[7] = (i01 * H[6] + i11 * H[7]) + i12 * H[8];
    o[8] = (i02 * H[6] + i12 * H[7]) + i22 * H[8];
}

// One wavefront per task.  Tasks [0, n_pairs): block (i, j) of the reduced system, Hschur = Hpp + lambda I - sum (W_a Dinv) W_b^T
// (block_solver.hpp:407,429), written to the LOWER triangle of S (the transposed block for i < j; of a diagonal block the upper
// triangle's values).  Tasks after them: bschur of free KeyFrame i = bp - sum W_e db (:413, :436-439).
static __global__ __launch_bounds__(kEdgeThreads) void ba_schur_kernel(const BaDev A, double lambda) {
    const size_t E = (size_t)A.E;
    const int task = blockIdx.x * (kEdgeThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (task >= A.n_pairs + A.Kf) return;
    if (task >= A.n_pairs) {
        const int i = task - A.n_pairs;
        double c[6] = {0, 0, 0, 0, 0, 0};
        for (int m = A.kf_begin[i] + lane; m < A.kf_begin[i + 1]; m += 64) {
            const int e = A.kf_edge[m];
            const double* db = A.Dinv + 9 * (size_t)A.edge_pt[e] + 6;
#pragma unroll
            for (int r = 0; r < 6; r++) {
                const double* W = A.lin + (size_t)(kW + 3 * r) * E + e;
                c[r] += (W[0] * db[0] + W[E] * db[1]) + W[2 * E] * db[2];
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
            for (int r = 0; r < 6; r++) c[r] += shfl_xor_f64(c[r], off);
        if (lane == 0)
#pragma unroll
            for (int r = 0; r < 6; r++) A.bs[6 * i + r] = A.Hpp[27 * (size_t)i + 21 + r] - c[r];
        return;
    }
    const int i = A.pair_i[task], j = A.pair_j[task];
    double T[36];
#pragma unroll
    for (int q = 0; q < 36; q++) T[q] = 0;
    for (int m = A.pair_begin[task] + lane; m < A.pair_begin[task + 1]; m += 64) {
        const int a = A.pair_a[m], b = A.pair_b[m];
        const double* Di = A.Dinv + 9 * (size_t)A.edge_pt[a];
        const double d00 = Di[0], d01 = Di[1], d02 = Di[2], d11 = Di[3], d12 = Di[4], d22 = Di[5];
        double Wb[6][3];
#pragma unroll
        for (int c = 0; c < 6; c++)
#pragma unroll
            for (int k = 0; k < 3; k++) Wb[c][k] = A.lin[(size_t)(kW + 3 * c + k) * E + b];
#pragma unroll
        for (int r = 0; r < 6; r++) {
            const double w0 = A.lin[(size_t)(kW + 3 * r) * E + a], w1 = A.lin[(size_t)(kW + 3 * r + 1) * E + a],
                         w2 = A.lin[(size_t)(kW + 3 * r + 2) * E + a];
            const double y0 = (w0 * d00 + w1 * d01) + w2 * d02, y1 = (w0 * d01 + w1 * d11) + w2 * d12,
                         y2 = (w0 * d02 + w1 * d12) + w2 * d22;   // BDinv = Bi Dinv
#pragma unroll
            for (int c = 0; c < 6; c++) T[6 * r + c] += (y0 * Wb[c][0] + y1 * Wb[c][1]) + y2 * Wb[c][2];
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int q = 0; q < 36; q++) T[q] += shfl_xor_f64(T[q], off);
    if (lane != 0) return;
    const size_t n = (size_t)A.n;
    if (i == j) {
        const double* H = A.Hpp + 27 * (size_t)i;
        int q = 0;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = r; c < 6; c++, q++) {
                double h = H[q];
                if (r == c) h += lambda;                                            // setLambda (block_solver.hpp:573-578)
                A.S[(size_t)(6 * i + c) * n + 6 * i + r] = h - T[6 * r + c];
            }
    } else {
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = 0; c < 6; c++) A.S[(size_t)(6 * j + c) * n + 6 * i + r] = 0.0 - T[6 * r + c];
    }
}

// SparseOptimizer::update of the state copy `from` into the copy `to` (sparse_optimizer.cpp:422-441), one thread per vertex: a
// free KeyFrame's oplus, and per point  xl = Dinv (bl - sum_e W_e^T xp)  (block_solver.hpp:461-481) with point += xl.  Each returns
// its terms of computeScale.
static __global__ __launch_bounds__(kEdgeThreads) void ba_update_kernel(const BaDev A, int from, int to, double lambda) {
    const size_t E = (size_t)A.E;
    const int v = blockIdx.x * kEdgeThreads + threadIdx.x;
    if (v < A.Kf) {
        const int k = A.kf_of_free[v];
        double x[6], sc = 0;
        for (int r = 0; r < 6; r++) {
            x[r] = A.x[6 * v + r];
            sc += x[r] * (lambda * x[r] + A.Hpp[27 * (size_t)v + 21 + r]);
        }
        const Pose N = oplus(load_pose(A.pose[from] + 7 * (size_t)k), x);
        double* o = A.pose[to] + 7 * (size_t)k;
        o[0] = N.qx; o[1] = N.qy; o[2] = N.qz; o[3] = N.qw; o[4] = N.tx; o[5] = N.ty; o[6] = N.tz;
        A.part_vtx[v] = sc;
        return;
    }
    const int p = v - A.Kf;
    if (p >= A.P) return;
    const double* H = A.Hll + 9 * (size_t)p;
    double cl[3] = {H[6], H[7], H[8]};
    for (int e = A.point_begin[p]; e < A.point_begin[p + 1]; e++) {
        const int i = A.free_of_kf[A.edge_kf[e]];
        if (i < 0) continue;
        const double* xp = A.x + 6 * (size_t)i;
#pragma unroll
        for (int c = 0; c < 3; c++) {   // cl += W^T (-xp) (SparseBlockMatrixCCS::rightMultiply)
            double tsum = 0;
#pragma unroll
            for (int r = 0; r < 6; r++) tsum += A.lin[(size_t)(kW + 3 * r + c) * E + e] * (-xp[r]);
            cl[c] += tsum;
        }
    }
    const double* D = A.Dinv + 9 * (size_t)p;
    double xl[3];
    xl[0] = (D[0] * cl[0] + D[1] * cl[1]) + D[2] * cl[2];
    xl[1] = (D[1] * cl[0] + D[3] * cl[1]) + D[4] * cl[2];
    xl[2] = (D[2] * cl[0] + D[4] * cl[1]) + D[5] * cl[2];
    double sc = 0;
    for (int c = 0; c < 3; c++) {
        sc += xl[c] * (lambda * xl[c] + H[6 + c]);
        A.pt[to][3 * (size_t)p + c] = A.pt[from][3 * (size_t)p + c] + xl[c];   // VertexSBAPointXYZ::oplusImpl
    }
    A.part_vtx[v] = sc;
}

// The two classifications of the welding bundle adjustment (Optimizer.cc:3726-3753, :3769-3803), which call no computeError():
// chi2() is what the last computeActiveErrors() left, the errors at the last trial's state (copy s_trial, which pop() has dropped
// if the trial was rejected), compared in double; isDepthPositive() reads the vertices, the estimate (copy s_cur).  chi_flag [E]
// keeps chi2 > threshold between the two: an edge is refreshed only where the last optimize() computed its error (refresh != 0
// and the edge is not on level 1), so a level-1 edge's flag stays what round 1 found.  out = chi_flag or the depth is not positive.
static __global__ __launch_bounds__(kEdgeThreads) void ba_classify_welding_kernel(const BaDev A, int s_trial, int s_cur, int refresh,
                                                                                  const uint8_t* level, uint8_t* chi_flag, uint8_t* out) {
    const int e = blockIdx.x * kEdgeThreads + threadIdx.x;
    if (e >= A.E) return;
    int k, p;
    uint8_t c = chi_flag[e];
    if (refresh && !(level && level[e])) {
        const EdgeGeom t = edge_geom(A, s_trial, e, k, p);
        c = t.chi2 > (t.stereo ? 7.815 : 5.991) ? 1 : 0;
        chi_flag[e] = c;
    }
    const EdgeGeom g = edge_geom(A, s_cur, e, k, p);
    out[e] = (c || !(g.z > 0.0)) ? 1 : 0;
}

// MSORB_LOCAL_BA_STAGES=1 (read once per process): every stage of a call is bracketed by two events, and
// msorb_local_ba_stage_ms returns the calling thread's last split.  Off, the call records no event but the two of elapsed_ms.
enum Stage { kLinearise, kSchur, kSolve, kTrial, kStages };
struct StageTimer {
    std::vector<hipEvent_t> pool;
    std::vector<int> stage;
    size_t used = 0;
    float ms[kStages] = {0, 0, 0, 0};
    hipError_t mark(int st, hipStream_t s) {   // called before and after a stage
        if (used == pool.size()) {
            hipEvent_t e;
            if (hipError_t err = hipEventCreate(&e)) return err;
            pool.push_back(e);
            stage.push_back(0);
        }
        stage[used] = st;
        return hipEventRecord(pool[used++], s);
    }
    hipError_t collect() {                      // after the stream has been synchronised
        for (float& v : ms) v = 0;
        for (size_t i = 0; i + 1 < used; i += 2) {
            float t = 0;
            if (hipError_t err = hipEventElapsedTime(&t, pool[i], pool[i + 1])) return err;
            ms[stage[i]] += t;
        }
        used = 0;
        return hipSuccess;
    }
};
static thread_local StageTimer g_stages;   // (its events live until the process ends)
inline bool stages_on() {
    static const bool on = [] { const char* e = getenv("MSORB_LOCAL_BA_STAGES"); return e && e[0] == '1'; }();
    return on;
}

struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at += up16(bytes); return o; }
};

}  // namespace ba
}  // namespace msorb
