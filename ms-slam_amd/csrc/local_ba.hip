// Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1040-1407) for pinhole KeyFrames without a second camera: g2o's
// Levenberg-Marquardt over KeyFrame poses and map points with the points eliminated by the Schur complement
// (core/block_solver.hpp:354-486), in double, then the classification of :1331-1373.  DESIGN.md section 10 has the whole story.
//
// The host drives the loop (optimization_algorithm_levenberg.cpp:61-170, sparse_optimizer.cpp:376-389) and reads 32 bytes back
// per linearisation and per trial: the cost, computeScale and the solver's status.  That is where the stop flag is looked at,
// exactly where g2o calls terminate().  Everything else stays on the device between the upload and the read-back of the result.
//
//   linearise   one thread per edge: error, Huber weight, both Jacobians, and the edge's terms of Hll / bl (point), Hpp / bp
//               (KeyFrame) and W = Hpl (6x3), written edge-major as 54 planes of E doubles; the cost as one partial per workgroup
//   gather      one thread per point adds its edges' Hll / bl terms (the edges are point-major: a contiguous run); one wavefront
//               per free KeyFrame adds Hpp / bp over the by-KeyFrame list (lane l takes entries l, l + 64, ...; xor butterfly)
//   trial       per lambda: D^-1 = adj(Hll + lambda I) / det and D^-1 bl per point; one wavefront per block pair (i, j) of the
//               reduced system adds W_a D^-1 W_b^T over the pair's list and one per KeyFrame adds W D^-1 bl; ONE workgroup factors
//               the dense 6 Kf x 6 Kf system (L D L^T, no pivoting, no square root) and substitutes; one thread per vertex applies
//               the update to a second copy of the state (push / pop is which copy is current) and returns its share of
//               computeScale; the errors at the trial state; a one-workgroup reduction of the cost and the scale.
//
// No floating-point atomics: every sum walks an index list of local_ba_plan.h in a fixed order, two runs return the same bits.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/msorb.h"
#include "hip_host.h"
#include "local_ba_plan.h"
#include "se3_device.h"

using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::up16;
using namespace msorb::se3;

namespace {

constexpr int kCapacity = 128;              // free KeyFrames: the reduced system is at most 768 x 768
constexpr int kMaxN = 6 * kCapacity;
constexpr int kEdgeThreads = 256, kSolveThreads = 1024;
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
        huber(g.chi2, (double)(g.stereo ? A.d_stereo : A.d_mono), true, rho0, rho1);
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
__global__ __launch_bounds__(kEdgeThreads) void ba_gather_kernel(const BaDev A, int point_blocks) {
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
__global__ __launch_bounds__(kEdgeThreads) void ba_finalize_kernel(const BaDev A, int vtx) {
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
__global__ __launch_bounds__(kEdgeThreads) void ba_point_inverse_kernel(const BaDev A, double lambda) {
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
__global__ __launch_bounds__(kEdgeThreads) void ba_schur_kernel(const BaDev A, double lambda) {
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

// The reduced system, dense: S = L D L^T without pivoting and without a square root (one reciprocal per pivot), right-looking over
// the lower triangle, then the two substitutions.  One workgroup; S stays in global memory (L2), a column and its scaled copy in
// LDS.  Column m's update of entry (i, k) is  - L[i][m] (L[k][m] D[m]),  applied for m ascending: the subtractions of the
// left-looking form of DESIGN section 9 in the same order.  A pivot that is not positive: solver_ok = 0, x untouched.
__global__ __launch_bounds__(kSolveThreads) void ba_solve_kernel(const BaDev A) {
    __shared__ double v[kMaxN], l[kMaxN], y[kMaxN], rd[kMaxN];
    const int n = A.n, t = threadIdx.x;
    double* S = A.S;
    for (int j = 0; j < n; j++) {
        const double d = S[(size_t)j * n + j];   // (uniform: every thread reads the same word, written before the last barrier)
        if (!(d > 0)) {
            if (t == 0) A.res->solver_ok = 0;
            return;
        }
        const double r = 1.0 / d;
        if (t == 0) rd[j] = r;
        for (int i = j + 1 + t; i < n; i += kSolveThreads) {
            const double s = S[(size_t)i * n + j];
            v[i] = s;
            l[i] = s * r;
            S[(size_t)i * n + j] = s * r;
        }
        __syncthreads();
        // the trailing lower triangle: a wavefront takes rows, its lanes the columns of a row
        for (int i = j + 1 + (t >> 6); i < n; i += kSolveThreads / 64) {
            const double li = l[i];
            double* row = S + (size_t)i * n;
            for (int k = j + 1 + (t & 63); k <= i; k += 64) row[k] -= li * v[k];
        }
        __syncthreads();
    }
    // L y = b: column by column, so y[i] loses L[i][m] y[m] for m ascending
    for (int i = t; i < n; i += kSolveThreads) y[i] = A.bs[i];
    __syncthreads();
    for (int m = 0; m < n; m++) {
        const double ym = y[m];
        __syncthreads();
        for (int i = m + 1 + t; i < n; i += kSolveThreads) y[i] -= S[(size_t)i * n + m] * ym;
        __syncthreads();
    }
    // D L^T x = y: x[i] = y[i] / D[i] - sum_m L[m][i] x[m], the columns taken from the last
    for (int i = t; i < n; i += kSolveThreads) y[i] *= rd[i];
    __syncthreads();
    for (int m = n - 1; m >= 0; m--) {
        const double xm = y[m];
        __syncthreads();
        for (int i = t; i < m; i += kSolveThreads) y[i] -= S[(size_t)m * n + i] * xm;
        __syncthreads();
    }
    for (int i = t; i < n; i += kSolveThreads) A.x[i] = y[i];
    if (t == 0) A.res->solver_ok = 1;
}

// SparseOptimizer::update of the state copy `from` into the copy `to` (sparse_optimizer.cpp:422-441), one thread per vertex: a
// free KeyFrame's oplus, and per point  xl = Dinv (bl - sum_e W_e^T xp)  (block_solver.hpp:461-481) with point += xl.  Each returns
// its terms of computeScale.
__global__ __launch_bounds__(kEdgeThreads) void ba_update_kernel(const BaDev A, int from, int to, double lambda) {
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

// :1331-1373: computeError at the final estimate, float fChi2 > 5.991 / 7.815 (double literals) or !isDepthPositive()
__global__ __launch_bounds__(kEdgeThreads) void ba_classify_kernel(const BaDev A, int s) {
    const int e = blockIdx.x * kEdgeThreads + threadIdx.x;
    if (e >= A.E) return;
    int k, p;
    const EdgeGeom g = edge_geom(A, s, e, k, p);
    const double c = (double)(float)g.chi2;
    A.outlier[e] = (c > (g.stereo ? 7.815 : 5.991) || !(g.z > 0.0)) ? 1 : 0;
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
thread_local StageTimer g_stages;   // (its events live until the process ends)
bool stages_on() {
    static const bool on = [] { const char* e = getenv("MSORB_LOCAL_BA_STAGES"); return e && e[0] == '1'; }();
    return on;
}

struct Carve {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at += up16(bytes); return o; }
};

}  // namespace

extern "C" int msorb_local_ba_capacity(void) { return kCapacity; }

extern "C" int msorb_local_ba_stage_ms(float ms[4]) {
    if (!ms) return MSORB_E_ARG;
    for (int i = 0; i < kStages; i++) ms[i] = g_stages.ms[i];
    return stages_on() ? MSORB_OK : MSORB_E_ARG;
}

extern "C" int msorb_local_ba(int device, int n_kf, const msorb_ba_keyframe* kfs, int n_points, const float* pos_w, int n_edges,
                              const int* edge_kf, const int* edge_point, const float* xy, const float* u_right, const float* inv_sigma2,
                              int max_iterations, const volatile int* stop_flag, float* kf_qt_out, double* kf_qt_d, float* pos_out,
                              double* pos_d, uint8_t* edge_outlier, msorb_ba_result* r, float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (!r || n_kf < 0 || n_points < 0 || n_edges < 0 || max_iterations < 0) return MSORB_E_ARG;
    if ((n_kf > 0 && (!kfs || !kf_qt_out)) || (n_points > 0 && (!pos_w || !pos_out)) ||
        (n_edges > 0 && (!edge_kf || !edge_point || !xy || !u_right || !inv_sigma2 || !edge_outlier)))
        return MSORB_E_ARG;
    std::memset(r, 0, sizeof *r);
    const int K = n_kf, P = n_points, E = n_edges;
    // what "nothing touched" returns: the inputs
    auto outputs_from_inputs = [&] {
        for (int k = 0; k < K; k++)
            for (int c = 0; c < 7; c++) {
                const float v = c < 4 ? kfs[k].q[c] : kfs[k].t[c - 4];
                kf_qt_out[7 * (size_t)k + c] = v;
                if (kf_qt_d) kf_qt_d[7 * (size_t)k + c] = (double)v;
            }
        for (size_t i = 0; i < 3 * (size_t)P; i++) {
            pos_out[i] = pos_w[i];
            if (pos_d) pos_d[i] = (double)pos_w[i];
        }
        if (E) std::memset(edge_outlier, 0, (size_t)E);
    };
    static thread_local std::vector<int> fixed;
    static thread_local msorb::LocalBaPlan plan;
    fixed.resize((size_t)K);
    for (int k = 0; k < K; k++) fixed[k] = kfs[k].fixed != 0;
    switch (msorb::build_local_ba_plan(K, fixed.data(), P, E, edge_kf, edge_point, plan)) {
        case msorb::kPlanIndexOutOfRange: set_last_error("local_ba: an edge names a KeyFrame or a point out of range"); return MSORB_E_ARG;
        case msorb::kPlanNotPointMajor: set_last_error("local_ba: the edges are not point-major"); return MSORB_E_ARG;
        default: break;
    }
    const int Kf = plan.Kf, n = 6 * Kf;
    if (Kf > kCapacity) {
        set_last_error("local_ba: more free KeyFrames than msorb_local_ba_capacity()");
        return MSORB_E_CAPACITY;
    }
    if (Kf == K) {   // :1098-1102
        r->status = 1;
        outputs_from_inputs();
        return MSORB_OK;
    }
    if (stop_flag && *stop_flag) {   // :1323-1325
        r->status = 2;
        outputs_from_inputs();
        return MSORB_OK;
    }
    if (int rc = msorb::require_device(device)) return rc;

    // ---- the device block: [uploaded | state and workspaces | results]
    const int n_pairs = (int)plan.pair_i.size(), n_blocks = (E + kEdgeThreads - 1) / kEdgeThreads;
    const size_t n_entries = plan.pair_a.size();
    Carve c;
    const size_t o_kf = c.take((size_t)K * sizeof(msorb_ba_keyframe)), o_free = c.take((size_t)K * 4), o_kof = c.take((size_t)Kf * 4);
    const size_t o_ekf = c.take((size_t)E * 4), o_ept = c.take((size_t)E * 4), o_pb = c.take(((size_t)P + 1) * 4);
    const size_t o_kb = c.take(((size_t)Kf + 1) * 4), o_ke = c.take(plan.kf_edge.size() * 4);
    const size_t o_prb = c.take(((size_t)n_pairs + 1) * 4), o_pi = c.take((size_t)n_pairs * 4), o_pj = c.take((size_t)n_pairs * 4);
    const size_t o_pa = c.take(n_entries * 4), o_pbb = c.take(n_entries * 4);
    const size_t o_xy = c.take((size_t)E * 8), o_ur = c.take((size_t)E * 4), o_w = c.take((size_t)E * 4);
    const size_t o_pose0 = c.take((size_t)K * 56), o_pt0 = c.take((size_t)P * 24);
    const size_t in_bytes = c.at;
    const size_t o_pose1 = c.take((size_t)K * 56), o_pt1 = c.take((size_t)P * 24);
    const size_t o_lin = c.take((size_t)kPlanes * E * 8), o_hpp = c.take((size_t)Kf * 27 * 8), o_hll = c.take((size_t)P * 72);
    const size_t o_dinv = c.take((size_t)P * 72), o_S = c.take((size_t)n * n * 8), o_bs = c.take((size_t)n * 8), o_x = c.take((size_t)n * 8);
    const size_t o_pc = c.take((size_t)n_blocks * 8), o_pv = c.take(((size_t)Kf + P) * 8);
    const size_t o_res = c.take(sizeof(BaRes)), o_out = c.take((size_t)E);
    const size_t dev_bytes = c.at;
    // pinned: the upload, then [res | pose | points | outlier] for the read-backs
    Carve hc;
    hc.at = in_bytes;
    const size_t h_res = hc.take(sizeof(BaRes)), h_pose = hc.take((size_t)K * 56), h_pt = hc.take((size_t)P * 24), h_out = hc.take((size_t)E);
    static thread_local ThreadScratch scr(true, 2);
    if (int rc = scr.acquire(device, dev_bytes, hc.at)) return rc;
    uint8_t *const h = scr.h.p, *const d = scr.d.p;
    hipStream_t s = scr.s;
    auto put = [&](size_t off, const void* src, size_t bytes) { if (bytes) std::memcpy(h + off, src, bytes); };
    put(o_kf, kfs, (size_t)K * sizeof(msorb_ba_keyframe));
    put(o_free, plan.free_of_kf.data(), (size_t)K * 4);
    put(o_kof, plan.kf_of_free.data(), (size_t)Kf * 4);
    put(o_ekf, edge_kf, (size_t)E * 4);
    put(o_ept, edge_point, (size_t)E * 4);
    put(o_pb, plan.point_begin.data(), ((size_t)P + 1) * 4);
    put(o_kb, plan.kf_begin.data(), ((size_t)Kf + 1) * 4);
    put(o_ke, plan.kf_edge.data(), plan.kf_edge.size() * 4);
    put(o_prb, plan.pair_begin.data(), ((size_t)n_pairs + 1) * 4);
    put(o_pi, plan.pair_i.data(), (size_t)n_pairs * 4);
    put(o_pj, plan.pair_j.data(), (size_t)n_pairs * 4);
    put(o_pa, plan.pair_a.data(), n_entries * 4);
    put(o_pbb, plan.pair_b.data(), n_entries * 4);
    put(o_xy, xy, (size_t)E * 8);
    put(o_ur, u_right, (size_t)E * 4);
    put(o_w, inv_sigma2, (size_t)E * 4);
    {   // :1134, :1150: the float pose widened, SE3Quat's constructor normalises (se3quat.h:62-64); :1200
        double* hp = reinterpret_cast<double*>(h + o_pose0);
        for (int k = 0; k < K; k++) {
            double q[4];
            for (int a = 0; a < 4; a++) q[a] = (double)kfs[k].q[a];
            if (q[3] < 0) for (int a = 0; a < 4; a++) q[a] *= -1;
            const double nrm = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
            for (int a = 0; a < 4; a++) hp[7 * (size_t)k + a] = q[a] / nrm;
            for (int a = 0; a < 3; a++) hp[7 * (size_t)k + 4 + a] = (double)kfs[k].t[a];
        }
        double* hx = reinterpret_cast<double*>(h + o_pt0);
        for (size_t i = 0; i < 3 * (size_t)P; i++) hx[i] = (double)pos_w[i];
    }
    BaDev A{};
    A.K = K; A.Kf = Kf; A.P = P; A.E = E; A.n = n; A.n_pairs = n_pairs; A.n_blocks = n_blocks;
    A.kf = reinterpret_cast<const msorb_ba_keyframe*>(d + o_kf);
    auto ip = [&](size_t off) { return reinterpret_cast<const int*>(d + off); };
    auto dp = [&](size_t off) { return reinterpret_cast<double*>(d + off); };
    A.free_of_kf = ip(o_free); A.kf_of_free = ip(o_kof); A.edge_kf = ip(o_ekf); A.edge_pt = ip(o_ept); A.point_begin = ip(o_pb);
    A.kf_begin = ip(o_kb); A.kf_edge = ip(o_ke); A.pair_begin = ip(o_prb); A.pair_i = ip(o_pi); A.pair_j = ip(o_pj);
    A.pair_a = ip(o_pa); A.pair_b = ip(o_pbb);
    A.xy = reinterpret_cast<const float*>(d + o_xy); A.ur = reinterpret_cast<const float*>(d + o_ur); A.w = reinterpret_cast<const float*>(d + o_w);
    A.pose[0] = dp(o_pose0); A.pose[1] = dp(o_pose1); A.pt[0] = dp(o_pt0); A.pt[1] = dp(o_pt1);
    A.lin = dp(o_lin); A.Hpp = dp(o_hpp); A.Hll = dp(o_hll); A.Dinv = dp(o_dinv); A.S = dp(o_S); A.bs = dp(o_bs); A.x = dp(o_x);
    A.part_cost = dp(o_pc); A.part_vtx = dp(o_pv);
    A.res = reinterpret_cast<BaRes*>(d + o_res);
    A.outlier = d + o_out;
    A.d_mono = (float)std::sqrt(5.991);
    A.d_stereo = (float)std::sqrt(7.815);

    hipError_t err = hipSuccess;
    auto fail = [&](const char* what) {
        set_last_error(std::string("local_ba: ") + what + ": " + hipGetErrorString(err));
        scr.release();
        return MSORB_E_HIP;
    };
#define BA_TRY(expr) do { err = (expr); if (err != hipSuccess) return fail(#expr); } while (0)
#define BA_LAUNCH(kernel, blocks, threads, ...)                                          \
    do {                                                                                 \
        if ((blocks) > 0) {                                                              \
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, s, __VA_ARGS__);  \
            BA_TRY(hipGetLastError());                                                   \
        }                                                                                \
    } while (0)
    const BaRes* hres = reinterpret_cast<const BaRes*>(h + h_res);
    auto read_res = [&]() -> hipError_t {
        hipError_t e2 = hipMemcpyAsync(h + h_res, d + o_res, sizeof(BaRes), hipMemcpyDeviceToHost, s);
        return e2 == hipSuccess ? hipStreamSynchronize(s) : e2;
    };
    const bool timed = stages_on();
    g_stages.used = 0;
#define BA_STAGE(st) do { if (timed) BA_TRY(g_stages.mark(st, s)); } while (0)
    const int point_blocks = (P + kEdgeThreads - 1) / kEdgeThreads, kf_blocks = (Kf + 3) / 4;
    const int vtx_blocks = (Kf + P + kEdgeThreads - 1) / kEdgeThreads, task_blocks = (n_pairs + Kf + 3) / 4;

    BA_TRY(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    // the second copy of the state starts equal to the first (a fixed KeyFrame is never written again)
    BA_TRY(hipMemcpyAsync(d + o_pose1, d + o_pose0, (size_t)K * 56, hipMemcpyDeviceToDevice, s));
    if (n) BA_TRY(hipMemsetAsync(d + o_x, 0, (size_t)n * 8, s));   // a failed first solve leaves x as it was: zero
    if (elapsed_ms) BA_TRY(hipEventRecord(scr.ev[0], s));

    int cur = 0;
    double lambda = 0, ni = 2;
    int n_bad = 0, iterations = 0, trials = 0, rejected = 0;
    auto stopped = [&] { return stop_flag && *stop_flag; };   // SparseOptimizer::terminate
    bool ok = E > 0;   // without an edge there is nothing to optimise: zero iterations, the estimates as they came
    for (int it = 0; it < max_iterations && !stopped() && ok; it++) {   // sparse_optimizer.cpp:376
        // ---- OptimizationAlgorithmLevenberg::solve (levenberg.cpp:61-170) ----
        BA_STAGE(kLinearise);
        BA_LAUNCH(ba_edges_kernel<true>, n_blocks, kEdgeThreads, A, cur);
        BA_LAUNCH(ba_gather_kernel, point_blocks + kf_blocks, kEdgeThreads, A, point_blocks);
        BA_LAUNCH(ba_finalize_kernel, 1, kEdgeThreads, A, it == 0 ? 1 : 0);
        BA_STAGE(kLinearise);
        BA_TRY(read_res());
        double current = hres->chi, temp = current;
        const double ini = current;
        if (it == 0) {   // :93-97, computeLambdaInit with _tau = 1e-5
            r->chi2_initial = current;
            lambda = 1e-5 * hres->max_diag;
            ni = 2;
            n_bad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            BA_STAGE(kSchur);
            BA_LAUNCH(ba_point_inverse_kernel, point_blocks, kEdgeThreads, A, lambda);   // :109-110
            if (n) BA_TRY(hipMemsetAsync(d + o_S, 0, (size_t)n * n * 8, s));   // the blocks no pair lists, which the last factorisation filled
            BA_LAUNCH(ba_schur_kernel, task_blocks, kEdgeThreads, A, lambda);
            BA_STAGE(kSchur);
            BA_STAGE(kSolve);
            if (n) BA_LAUNCH(ba_solve_kernel, 1, kSolveThreads, A);
            BA_STAGE(kSolve);
            BA_STAGE(kTrial);
            BA_LAUNCH(ba_update_kernel, vtx_blocks, kEdgeThreads, A, cur, cur ^ 1, lambda);   // push + update (:103, :115)
            BA_LAUNCH(ba_edges_kernel<false>, n_blocks, kEdgeThreads, A, cur ^ 1);            // :123-124
            BA_LAUNCH(ba_finalize_kernel, 1, kEdgeThreads, A, 2);
            BA_STAGE(kTrial);
            BA_TRY(read_res());
            temp = hres->chi;
            if (n && !hres->solver_ok) temp = DBL_MAX;   // :126-127
            rho = current - temp;
            const double scale = hres->scale + 1e-3;     // :130-131
            rho /= scale;
            trials++;
            if (rho > 0 && std::isfinite(temp)) {        // :134-142
                const double y = 2 * rho - 1;
                double alpha = 1. - (y * y) * y;
                alpha = std::fmin(alpha, 2. / 3.);
                lambda *= std::fmax(1. / 3., alpha);
                ni = 2;
                current = temp;
                cur ^= 1;                                // discardTop: the trial copy is the state
            } else {                                     // :143-147: pop = the trial copy is dropped
                lambda *= ni;
                ni *= 2;
                rejected++;
            }
            qmax++;
        } while (rho < 0 && qmax < 10 && !stopped());    // :149
        iterations++;
        r->chi2_final = current;
        if (qmax == 10 || rho == 0) { ok = false; continue; }   // :151-155
        if ((ini - current) * 1e3 < ini) n_bad++;               // :157-162
        else n_bad = 0;
        if (n_bad >= 3) ok = false;                             // :164-167
    }
    if (iterations == 0) r->chi2_final = r->chi2_initial;
    BA_LAUNCH(ba_classify_kernel, n_blocks, kEdgeThreads, A, cur);
    if (elapsed_ms) BA_TRY(hipEventRecord(scr.ev[1], s));
    BA_TRY(hipMemcpyAsync(h + h_pose, d + (cur ? o_pose1 : o_pose0), (size_t)K * 56, hipMemcpyDeviceToHost, s));
    if (P) BA_TRY(hipMemcpyAsync(h + h_pt, d + (cur ? o_pt1 : o_pt0), (size_t)P * 24, hipMemcpyDeviceToHost, s));
    if (E) BA_TRY(hipMemcpyAsync(h + h_out, d + o_out, (size_t)E, hipMemcpyDeviceToHost, s));
    BA_TRY(hipStreamSynchronize(s));
    if (elapsed_ms) BA_TRY(hipEventElapsedTime(elapsed_ms, scr.ev[0], scr.ev[1]));
    if (timed) BA_TRY(g_stages.collect());
#undef BA_STAGE
#undef BA_LAUNCH
#undef BA_TRY
    const double* hp = reinterpret_cast<const double*>(h + h_pose);
    for (int k = 0; k < K; k++)
        for (int a = 0; a < 7; a++) {
            const bool fx = fixed[k] != 0;   // a fixed KeyFrame's output repeats its input
            const float in = a < 4 ? kfs[k].q[a] : kfs[k].t[a - 4];
            kf_qt_out[7 * (size_t)k + a] = fx ? in : (float)hp[7 * (size_t)k + a];   // :1393
            if (kf_qt_d) kf_qt_d[7 * (size_t)k + a] = fx ? (double)in : hp[7 * (size_t)k + a];
        }
    const double* hx = reinterpret_cast<const double*>(h + h_pt);
    for (size_t i = 0; i < 3 * (size_t)P; i++) {
        pos_out[i] = (float)hx[i];   // :1402
        if (pos_d) pos_d[i] = hx[i];
    }
    int n_out = 0;
    for (int e = 0; e < E; e++) { edge_outlier[e] = h[h_out + e]; n_out += edge_outlier[e] != 0; }
    r->status = 0;
    r->iterations = iterations;
    r->trials = trials;
    r->rejected_trials = rejected;
    r->n_outliers = n_out;
    r->lambda_final = lambda;
    return MSORB_OK;
}
