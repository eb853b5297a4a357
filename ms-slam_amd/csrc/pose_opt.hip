// Optimizer::PoseOptimization (src/Optimizer.cc:759-1037) for pinhole mono / stereo frames: motion-only bundle adjustment of one
// 6-DoF vertex over N unary edges, the whole routine in ONE launch, in double like g2o.
//
// One workgroup of 256 threads owns a problem (blockIdx.x = problem).  Thread t owns the observations t, t + 256, t + 512, ...: up to
// kPerThread = 8 of them live in registers as the reference's floats (N <= kResident = 2048) and are widened where they are used;
// a longer problem walks the same indices in global memory, with the per-edge state (the stale chi2, the level) in a workspace.
// Both forms add in the same order, so the split is invisible in the result.
//
// A Levenberg step is a map over the active observations (project, error, Huber weight, Jacobian, the 27 sums of the upper triangle
// of H and of b, and the cost) and ONE reduction: every thread adds its observations in ascending index, a wavefront adds its 64
// partial sums by an xor butterfly (32, 16, 8, 4, 2, 1: every lane ends with the same bits), lane 0 of each wavefront writes its 28
// doubles to LDS, and after one barrier every thread adds the four wavefronts in ascending order.  The LDS block is double-buffered,
// so a reduction costs one barrier.  Every thread then holds H, b and the cost and runs the 6x6 L D L^T, SE3Quat::exp and the pose
// update redundantly: no second barrier, no broadcast.  A trial is a second map (errors only) and a one-value reduction.
// No atomics anywhere: two runs give the same bits.
//
// The stale-error rule (Optimizer.cc:959-963 with optimization_algorithm_levenberg.cpp:123,146): an inlier's chi2 at the
// classification is what the LAST computeActiveErrors left, i.e. the error at the last TRIAL pose, also when that trial was rejected
// and the pose popped.  Every pass therefore writes the edge's chi2 into its per-edge state, and the classification re-computes only
// the edges that are outliers at that moment.
//
// Two kernels share all of the above through one template over an edge model: pose_opt_kernel (PinholeModel: pFrame->fx ... mbf, mono
// and stereo edges, the arm :806-867) and pose_opt_rig_kernel (RigModel: the arm :870-931 and a one-camera frame whose camera is not
// a pinhole; mono edges through pCamera->project / projectJac of pose_rig_device.h, the right camera's through mTrl).  The pinhole
// instantiation is the kernel this file has always had: same registers, same private and LDS bytes, same result bits.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/msorb.h"
#include "hip_host.h"
#include "matcher_host.h"
#include "pose_rig_device.h"
#include "se3_device.h"

namespace msorb {
hipError_t small_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s);   // orb_kernels.hip
}
using msorb::KpLite;
using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::up16;
using namespace msorb::se3;

namespace {

constexpr int kThreads = 256, kPerThread = 8, kResident = kThreads * kPerThread, kWaves = kThreads / 64;
constexpr int kSums = 28;   // 21 (upper triangle of H, row major) + 6 (b) + 1 (the cost)

struct PoseProblemDev {
    msorb_pose_problem p;
    int obs0;   // first observation of the problem in the flat arrays
};
static_assert(sizeof(msorb_pose_problem) == 52 && sizeof(msorb_pose_result) == 128, "the records of include/msorb.h as the Python mirror lays them out");
struct PoseArgs {
    const PoseProblemDev* prob;
    // flat form: per observation
    const float* xy;
    const float* u_right;
    const float* inv_sigma2;
    const float* pos_w;
    // frame form: the handle's keypoint table, the indices of the keypoints that have a point (ascending), mvInvLevelSigma2
    const KpLite* kp;
    const int* kp_idx;
    float level_inv_sigma2[MSORB_MAX_LEVELS];
    float delta_mono, delta_stereo;   // (float)sqrt(5.991), (float)sqrt(7.815): Optimizer.cc:796-797
    double* chi2_ws;       // per observation, read and written by the problems with n > kResident only
    uint8_t* outlier;      // per observation: out (and the level of the strided form between the rounds)
    msorb_pose_result* result;
};

struct Ob { float x, y, ur, w, X, Y, Z; };   // one edge as the reference holds it before the widening (:814,:820,:828 / :842,:848,:861)
struct Cam { double fx, fy, cx, cy, bf; };

__device__ inline Ob load_ob(const PoseArgs& A, int i) {
    Ob o;
    if (A.kp) {
        const int k = A.kp_idx[i];
        const KpLite kp = A.kp[k];
        o.x = kp.x; o.y = kp.y; o.ur = kp.u_right;
        o.w = A.level_inv_sigma2[min(max(kp.octave, 0), MSORB_MAX_LEVELS - 1)];
    } else {
        o.x = A.xy[2 * (size_t)i]; o.y = A.xy[2 * (size_t)i + 1]; o.ur = A.u_right[i]; o.w = A.inv_sigma2[i];
    }
    o.X = A.pos_w[3 * (size_t)i]; o.Y = A.pos_w[3 * (size_t)i + 1]; o.Z = A.pos_w[3 * (size_t)i + 2];
    return o;
}

// computeError of the two edges -> e[3] (e[2] = 0 for a mono edge), the camera-frame point, and chi2() = e . (Omega e)
// (base_edge.h:60).  Stereo: types_six_dof_expmap.h:218-222 with cam_project (.cpp:339-346, whose invz is a FLOAT); mono:
// OptimizableTypes.h (obs - pCamera->project(map(Xw))) with Pinhole::project (Pinhole.cpp:35-41).
__device__ inline double edge_error(const Pose& T, const Cam& c, const Ob& o, double* e, double& x, double& y, double& z) {
    rotate(T, (double)o.X, (double)o.Y, (double)o.Z, x, y, z);
    x += T.tx; y += T.ty; z += T.tz;
    const double w = (double)o.w;
    if (o.ur >= 0) {
        const double invz = (double)(float)(1.0 / z);
        const double p0 = (x * invz) * c.fx + c.cx;
        e[0] = (double)o.x - p0;
        e[1] = (double)o.y - ((y * invz) * c.fy + c.cy);
        e[2] = (double)o.ur - (p0 - c.bf * invz);
        return (e[0] * (w * e[0]) + e[1] * (w * e[1])) + e[2] * (w * e[2]);
    }
    e[0] = (double)o.x - ((c.fx * x) / z + c.cx);
    e[1] = (double)o.y - ((c.fy * y) / z + c.cy);
    e[2] = 0;
    return e[0] * (w * e[0]) + e[1] * (w * e[1]);
}

// the edge's Jacobian: stereo types_six_dof_expmap.cpp:375-403; mono OptimizableTypes.cpp:49-63 with Pinhole::projectJac (Pinhole.cpp:71-81)
__device__ inline void edge_jacobian(const Cam& c, bool stereo, double x, double y, double z, double (*J)[6]) {
    if (stereo) {
        const double invz = 1.0 / z, invz_2 = invz * invz;
        J[0][0] = ((x * y) * invz_2) * c.fx;
        J[0][1] = -(1 + ((x * x) * invz_2)) * c.fx;
        J[0][2] = (y * invz) * c.fx;
        J[0][3] = -invz * c.fx;
        J[0][4] = 0;
        J[0][5] = (x * invz_2) * c.fx;
        J[1][0] = (1 + (y * y) * invz_2) * c.fy;
        J[1][1] = ((-x * y) * invz_2) * c.fy;
        J[1][2] = (-x * invz) * c.fy;
        J[1][3] = 0;
        J[1][4] = -invz * c.fy;
        J[1][5] = (y * invz_2) * c.fy;
        J[2][0] = J[0][0] - (c.bf * y) * invz_2;
        J[2][1] = J[0][1] + (c.bf * x) * invz_2;
        J[2][2] = J[0][2];
        J[2][3] = J[0][3];
        J[2][4] = 0;
        J[2][5] = J[0][5] - c.bf * invz_2;
    } else {
        const double a = c.fx / z, g = (-c.fx * x) / (z * z), b = c.fy / z, d = (-c.fy * y) / (z * z);
        // -(projectJac * [-[X]x | I]): rows of [0 z -y 1 0 0; -z 0 x 0 1 0; y -x 0 0 0 1]
        J[0][0] = -(g * y);         J[0][1] = -(a * z + g * -x); J[0][2] = -(a * -y); J[0][3] = -a; J[0][4] = 0;  J[0][5] = -g;
        J[1][0] = -(b * -z + d * y); J[1][1] = -(d * -x);         J[1][2] = -(b * x);  J[1][3] = 0;  J[1][4] = -b; J[1][5] = -d;
        for (int j = 0; j < 6; j++) J[2][j] = 0;
    }
}

// sums v[0, N) over the workgroup; every thread returns with the same bits.  `lds` is one of the two kWaves * kSums blocks; the
// caller alternates them, so the barrier below also protects the block of the reduction before the last.
template <int N>
__device__ inline void block_sum(double* v, double* lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int i = 0; i < N; i++) v[i] += shfl_xor_f64(v[i], off);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < N; i++) lds[wave * kSums + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; i++) {
        double s = lds[i];
        for (int w = 1; w < kWaves; w++) s += lds[w * kSums + i];
        v[i] = s;
    }
}

// Square-root-free Cholesky (L D L^T, no pivoting) of H + lambda I (the upper triangle in Hu, row major), then the substitutions.
// One reciprocal per pivot and no square root: the divisions are the long dependent chain of a step.  false = a pivot that is
// not positive (LinearSolverDense, an LDLT too, reports !isPositive(): the trial then counts as failed, levenberg.cpp:126-127)
// and x keeps what it held.
__device__ inline bool solve6(const double* Hu, double lambda, const double* b, double* x) {
    double L[6][6], r[6];
    int k = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) { L[j][i] = Hu[k++]; if (i == j) L[i][i] += lambda; }   // setLambda (block_solver.hpp)
    for (int j = 0; j < 6; j++) {
        double v[6];
        double d = L[j][j];
        for (int m = 0; m < j; m++) { v[m] = L[j][m] * L[m][m]; d -= L[j][m] * v[m]; }
        if (!(d > 0)) return false;
        L[j][j] = d;
        r[j] = 1.0 / d;
        for (int i = j + 1; i < 6; i++) {
            double s = L[i][j];
            for (int m = 0; m < j; m++) s -= L[i][m] * v[m];
            L[i][j] = s * r[j];
        }
    }
    double y[6];
    for (int i = 0; i < 6; i++) {
        double s = b[i];
        for (int m = 0; m < i; m++) s -= L[i][m] * y[m];
        y[i] = s;
    }
    for (int i = 5; i >= 0; i--) {
        double s = y[i] * r[i];
        for (int m = i + 1; m < 6; m++) s -= L[m][i] * x[m];
        x[i] = s;
    }
    return true;
}

// ---- the edge models.  pose_opt_problem below (the rounds, the Levenberg loop, the sums, the classification) is written once over
// a model M: its argument block and problem record, what it derives from the problem (Setup) and from a pose (AtPose), how an
// observation is loaded, whether an edge may have a third row, the error and the Jacobian.
struct PinholeModel {   // the arm :806-867: pFrame->fx ... mbf, mono and stereo edges
    typedef PoseArgs Args;
    typedef PoseProblemDev Problem;
    typedef Cam Setup;
    struct AtPose {};
    static constexpr int kPer = kPerThread;
    static constexpr bool kStereoEdges = true;    // u_right >= 0: a three-row edge (:808)
    __device__ static inline Setup setup(const Problem& P) {
        return Cam{(double)P.p.fx, (double)P.p.fy, (double)P.p.cx, (double)P.p.cy, (double)P.p.mbf};
    }
    __device__ static inline AtPose at_pose(const Setup&, const Pose&) { return AtPose{}; }
    __device__ static inline Ob load(const Args& A, int i) { return load_ob(A, i); }
    __device__ static inline double error(const Pose& T, const AtPose&, const Setup& c, const Ob& o, double* e, double& x, double& y, double& z) {
        return edge_error(T, c, o, e, x, y, z);
    }
    __device__ static inline void jacobian(const Setup& c, const Ob&, bool stereo, double x, double y, double z, double (*J)[6]) {
        edge_jacobian(c, stereo, x, y, z, J);
    }
};

// The arm :870-931 and a one-camera frame through pCamera->project: mono edges only, Ob.ur carries the camera (0 left, 1 right).
// kRigPerThread: the KannalaBrandt8 edge holds more live doubles than the pinhole one, but with the problem's uniform data in LDS (see
// setup) 8 observations per thread spill no VGPR (DESIGN.md section 28 has the compiler's figures), so the capacity is the pinhole's.
constexpr int kRigPerThread = 8;
struct RigProblemDev {
    msorb_pose_rig_problem p;
    int obs0;
};
static_assert(sizeof(msorb_camera_model) == 36 && sizeof(msorb_pose_rig_problem) == 136 && sizeof(msorb_camera_model) == sizeof(msorb::rig::Camera),
              "the records of include/msorb.h as the Python mirror lays them out");
struct RigArgs {
    const RigProblemDev* prob;
    const float* xy;
    const uint8_t* camera;
    const float* inv_sigma2;
    const float* pos_w;
    float delta_mono, delta_stereo;   // delta_stereo is never read: the arm has no stereo edge
    double* chi2_ws;
    uint8_t* outlier;
    msorb_pose_result* result;
};
struct RigModel {
    typedef RigArgs Args;
    typedef RigProblemDev Problem;
    struct Setup { const msorb::rig::Rig* g; };   // in LDS: uniform, read where an edge needs it, so it holds no registers between
    typedef Pose AtPose;   // mTrl * estimate, the product the right camera's computeError maps through
    static constexpr int kPer = kRigPerThread;
    static constexpr bool kStereoEdges = false;   // Ob.ur is the camera, not a coordinate
    __device__ static inline Setup setup(const Problem& P) {
        __shared__ msorb::rig::Rig g;
        if (threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c < 2; c++) {
                g.cam[c].type = P.p.cam[c].type;
#pragma unroll
                for (int k = 0; k < 8; k++) g.cam[c].p[k] = P.p.cam[c].p[k];
            }
            const float q1[4] = {0, 0, 0, 1}, t1[3] = {0, 0, 0};
            if (P.p.n_cameras == 2) msorb::rig::set_trl(g, P.p.q_rl, P.p.t_rl);
            else msorb::rig::set_trl(g, q1, t1);   // never read: no observation names the right camera
        }
        __syncthreads();
        return Setup{&g};
    }
    __device__ static inline AtPose at_pose(const Setup& s, const Pose& T) { return msorb::rig::compose(s.g->Trl, T); }
    __device__ static inline Ob load(const Args& A, int i) {
        Ob o;
        o.x = A.xy[2 * (size_t)i]; o.y = A.xy[2 * (size_t)i + 1]; o.ur = (float)A.camera[i]; o.w = A.inv_sigma2[i];
        o.X = A.pos_w[3 * (size_t)i]; o.Y = A.pos_w[3 * (size_t)i + 1]; o.Z = A.pos_w[3 * (size_t)i + 2];
        return o;
    }
    __device__ static inline double error(const Pose& T, const AtPose& Trw, const Setup& s, const Ob& o, double* e, double& x, double& y, double& z) {
        e[2] = 0;
        return msorb::rig::edge_error(*s.g, T, Trw, o.ur != 0, (double)o.x, (double)o.y, (double)o.w, (double)o.X, (double)o.Y, (double)o.Z, e, x, y, z);
    }
    __device__ static inline void jacobian(const Setup& s, const Ob& o, bool, double x, double y, double z, double (*J)[6]) {
        msorb::rig::edge_jacobian(*s.g, o.ur != 0, x, y, z, J);
    }
};

// per-edge state of the register-resident form
template <int PER>
struct Resident {
    Ob ob[PER];
    double chi2[PER];
    uint8_t level[PER];   // 1 = outlier (e->setLevel(1), Optimizer.cc:966-972)
};

// f(ob, chi2&, level&) over the thread's observations in ascending index
template <bool RES, typename M, typename F>
__device__ inline void for_each_edge(const typename M::Args& A, Resident<M::kPer>& r, int obs0, int n, F f) {
    if constexpr (RES) {
#pragma unroll
        for (int k = 0; k < M::kPer; k++)
            if ((int)threadIdx.x + k * kThreads < n) f(r.ob[k], r.chi2[k], r.level[k]);
    } else {
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const Ob o = M::load(A, obs0 + i);
            double chi2 = A.chi2_ws[obs0 + i];
            uint8_t level = A.outlier[obs0 + i];
            f(o, chi2, level);
            A.chi2_ws[obs0 + i] = chi2;
            A.outlier[obs0 + i] = level;
        }
    }
}

template <bool RES, typename M>
__device__ void pose_opt_problem(const typename M::Args& A, double* lds) {
    const typename M::Problem P = A.prob[blockIdx.x];
    const int n = P.p.n, obs0 = P.obs0;
    const typename M::Setup cam = M::setup(P);
    const double d_mono = (double)A.delta_mono, d_stereo = (double)A.delta_stereo;
    Resident<M::kPer> r;
    if constexpr (RES) {
#pragma unroll
        for (int k = 0; k < M::kPer; k++) {
            const int i = threadIdx.x + k * kThreads;
            r.ob[k] = i < n ? M::load(A, obs0 + i) : Ob{};
            r.chi2[k] = 0;
            r.level[k] = 0;
        }
    } else {
        for (int i = threadIdx.x; i < n; i += kThreads) { A.chi2_ws[obs0 + i] = 0; A.outlier[obs0 + i] = 0; }
    }
    // :774-775: the float pose widened, SE3Quat's constructor normalises
    Pose T0{(double)P.p.q[0], (double)P.p.q[1], (double)P.p.q[2], (double)P.p.q[3], (double)P.p.t[0], (double)P.p.t[1], (double)P.p.t[2]};
    normalize_rotation(T0);
    Pose T = T0;
    int iterations[4] = {-1, -1, -1, -1}, rejected[4] = {-1, -1, -1, -1};
    int n_bad = 0, n_active = n, buf = 0;
    double x[6] = {0, 0, 0, 0, 0, 0};
    for (int it = 0; it < 4; it++) {
        const bool robust = it < 3;   // :974-975: the kernel is dropped after the third classification
        T = T0;                       // :947-948
        int n_solve = 0, n_rejected = 0;
        if (n_active > 0) {           // sparse_optimizer.cpp:356-359
            double lambda = 0, ni = 2;
            int n_bad_steps = 0;
            bool ok = true;
            for (int i = 0; i < 10 && ok; i++) {   // sparse_optimizer.cpp:376, its[] = 10
                // ---- OptimizationAlgorithmLevenberg::solve (levenberg.cpp:61-170) ----
                double S[kSums];
#pragma unroll
                for (int k = 0; k < kSums; k++) S[k] = 0;
                const typename M::AtPose V = M::at_pose(cam, T);
                for_each_edge<RES, M>(A, r, obs0, n, [&](const Ob& o, double& chi2, uint8_t& level) {
                    if (level) return;
                    double e[3], px, py, pz, J[3][6], rho0, rho1;
                    // (the expression, not a function of the model taking `o`: that form cost the pinhole kernel 28 AGPRs)
                    const bool stereo = M::kStereoEdges && o.ur >= 0;
                    chi2 = M::error(T, V, cam, o, e, px, py, pz);       // computeActiveErrors (:75)
                    huber(chi2, stereo ? d_stereo : d_mono, robust, rho0, rho1);
                    S[27] += rho0;                                      // activeRobustChi2 (:82)
                    M::jacobian(cam, o, stereo, px, py, pz, J);         // buildSystem (:87): base_unary_edge.hpp:43-72
                    const double w = (double)o.w, wr = rho1 * w;        // robustInformation (base_edge.h:96-100)
                    int k = 0;
#pragma unroll
                    for (int a = 0; a < 6; a++) {
#pragma unroll
                        for (int c = a; c < 6; c++, k++) {
                            double t = (J[0][a] * wr) * J[0][c] + (J[1][a] * wr) * J[1][c];
                            if (stereo) t += (J[2][a] * wr) * J[2][c];
                            S[k] += t;
                        }
                        double t = ((rho1 * J[0][a]) * w) * e[0] + ((rho1 * J[1][a]) * w) * e[1];
                        if (stereo) t += ((rho1 * J[2][a]) * w) * e[2];
                        S[21 + a] -= t;
                    }
                });
                block_sum<kSums>(S, lds + (buf ^= 1) * kWaves * kSums);
                double current = S[27], temp = current;
                const double ini = current;
                const double* Hu = S;
                const double* b = S + 21;
                if (i == 0) {   // computeLambdaInit (:172-186), _tau = 1e-5
                    double max_diag = 0;
                    for (int j = 0, k = 0; j < 6; k += 6 - j, j++) max_diag = fmax(fabs(Hu[k]), max_diag);
                    lambda = 1e-5 * max_diag;
                    ni = 2;
                    n_bad_steps = 0;
                }
                double rho = 0;
                int qmax = 0;
                do {
                    const Pose backup = T;                       // push (:103)
                    const bool ok2 = solve6(Hu, lambda, b, x);   // :109-110
                    T = oplus(T, x);                             // :115
                    double c1[1] = {0};
                    const typename M::AtPose Vt = M::at_pose(cam, T);
                    for_each_edge<RES, M>(A, r, obs0, n, [&](const Ob& o, double& chi2, uint8_t& level) {
                        if (level) return;
                        double e[3], px, py, pz, rho0, rho1;
                        chi2 = M::error(T, Vt, cam, o, e, px, py, pz);   // :123
                        huber(chi2, M::kStereoEdges && o.ur >= 0 ? d_stereo : d_mono, robust, rho0, rho1);
                        c1[0] += rho0;                                 // :124
                    });
                    block_sum<1>(c1, lds + (buf ^= 1) * kWaves * kSums);
                    temp = c1[0];
                    if (!ok2) temp = DBL_MAX;   // :126-127
                    rho = current - temp;
                    double scale = 0;           // computeScale (:188-195)
                    for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + b[j]);
                    scale += 1e-3;
                    rho /= scale;
                    if (rho > 0 && isfinite(temp)) {   // :134-142
                        const double y = 2 * rho - 1;
                        double alpha = 1. - (y * y) * y;   // pow(2 rho - 1, 3)
                        alpha = fmin(alpha, 2. / 3.);
                        const double factor = fmax(1. / 3., alpha);
                        lambda *= factor;
                        ni = 2;
                        current = temp;
                    } else {                           // :143-147
                        lambda *= ni;
                        ni *= 2;
                        T = backup;
                        n_rejected++;
                    }
                    qmax++;
                } while (rho < 0 && qmax < 10);   // :149
                n_solve++;
                if (qmax == 10 || rho == 0) { ok = false; continue; }   // :151-155 Terminate
                if ((ini - current) * 1e3 < ini) n_bad_steps++;         // :157-162
                else n_bad_steps = 0;
                if (n_bad_steps >= 3) ok = false;                       // :164-167
            }
        }
        iterations[it] = n_solve;
        rejected[it] = n_rejected;
        // ---- the classification (Optimizer.cc:953-1024) ----
        double bad[1] = {0};
        const typename M::AtPose Vc = M::at_pose(cam, T);
        for_each_edge<RES, M>(A, r, obs0, n, [&](const Ob& o, double& chi2, uint8_t& level) {
            const bool stereo = M::kStereoEdges && o.ur >= 0;
            if (level) {   // :959-961, :1007-1009 (:983-985 for the right camera's edges)
                double e[3], px, py, pz;
                chi2 = M::error(T, Vc, cam, o, e, px, py, pz);
            }
            const float c = (float)chi2;   // :963, :1011
            level = c > (stereo ? 7.815f : 5.991f) ? 1 : 0;
            bad[0] += level;
        });
        block_sum<1>(bad, lds + (buf ^= 1) * kWaves * kSums);
        n_bad = (int)bad[0];
        n_active = n - n_bad;
        if (n < 10) break;   // :1026-1027
    }
    if constexpr (RES) {
#pragma unroll
        for (int k = 0; k < M::kPer; k++) {
            const int i = threadIdx.x + k * kThreads;
            if (i < n) A.outlier[obs0 + i] = r.level[k];
        }
    }
    if (threadIdx.x == 0) {
        msorb_pose_result& R = A.result[blockIdx.x];
        R.qd[0] = T.qx; R.qd[1] = T.qy; R.qd[2] = T.qz; R.qd[3] = T.qw;
        R.td[0] = T.tx; R.td[1] = T.ty; R.td[2] = T.tz;
        for (int k = 0; k < 4; k++) R.q[k] = (float)R.qd[k];   // :1033-1034
        for (int k = 0; k < 3; k++) R.t[k] = (float)R.td[k];
        R.n_initial = n;
        R.n_bad = n_bad;
        for (int k = 0; k < 4; k++) { R.iterations[k] = iterations[k]; R.rejected_trials[k] = rejected[k]; }
    }
}

template <typename M>
__device__ inline void pose_opt_block(const typename M::Args& A, double* lds) {
    const int n = A.prob[blockIdx.x].p.n;
    if (n < 3) {   // :936-937: return 0, the frame's pose as it was, the flags cleared by the gathering loop (:810, :837, :878, :907)
        const typename M::Problem P = A.prob[blockIdx.x];
        for (int i = threadIdx.x; i < n; i += kThreads) A.outlier[P.obs0 + i] = 0;
        if (threadIdx.x == 0) {
            msorb_pose_result& R = A.result[blockIdx.x];
            for (int k = 0; k < 4; k++) { R.q[k] = P.p.q[k]; R.qd[k] = (double)P.p.q[k]; R.iterations[k] = -1; R.rejected_trials[k] = -1; }
            for (int k = 0; k < 3; k++) { R.t[k] = P.p.t[k]; R.td[k] = (double)P.p.t[k]; }
            R.n_initial = n;
            R.n_bad = n;   // n_initial - n_bad = the 0 the reference returns
        }
        return;
    }
    if (n <= M::kPer * kThreads) pose_opt_problem<true, M>(A, lds);
    else pose_opt_problem<false, M>(A, lds);
}

__global__ __launch_bounds__(kThreads) void pose_opt_kernel(const PoseArgs A) {
    __shared__ double lds[2 * kWaves * kSums];
    pose_opt_block<PinholeModel>(A, lds);
}

__global__ __launch_bounds__(kThreads) void pose_opt_rig_kernel(const RigArgs A) {
    __shared__ double lds[2 * kWaves * kSums];
    pose_opt_block<RigModel>(A, lds);
}

int hip_fail(ThreadScratch& scr, const char* what, hipError_t e) {
    set_last_error(std::string(what) + ": " + hipGetErrorString(e));
    scr.release();
    return MSORB_E_HIP;
}

// One upload, one launch, one read-back on the calling thread's scratch.  Staging: [problems | idx or (xy | u_right | inv_sigma2) |
// pos_w] up, [results | outlier] down, then the chi2 workspace of the problems above kResident.
struct Staged {
    int n_problems;
    size_t total;   // observations
    bool frame;
    size_t o_prob, o_a, o_ur, o_inv, o_pos, in_bytes, o_res, o_out, o_ws, dev_bytes, pin_bytes;
    Staged(int np, size_t tot, bool fr, bool strided) : n_problems(np), total(tot), frame(fr) {
        o_prob = 0;
        o_a = up16((size_t)np * sizeof(PoseProblemDev));
        if (fr) { o_ur = o_inv = o_a; o_pos = o_a + up16(tot * 4); }
        else { o_ur = o_a + up16(tot * 8); o_inv = o_ur + up16(tot * 4); o_pos = o_inv + up16(tot * 4); }
        in_bytes = o_pos + up16(tot * 12);
        o_res = in_bytes;
        o_out = o_res + up16((size_t)np * sizeof(msorb_pose_result));
        o_ws = o_out + up16(tot);
        pin_bytes = o_ws;
        dev_bytes = o_ws + (strided ? tot * 8 : 0);
    }
};

// the upload [0, in_bytes), the launch of one workgroup per problem, the read-back [o_res, o_end), the synchronisation
template <typename ArgsT>
int launch_staged(ThreadScratch& scr, void (*kernel)(const ArgsT), const ArgsT& A, int n_problems, size_t in_bytes, size_t o_res, size_t o_end, hipStream_t after,
                  float* elapsed_ms) {
    uint8_t *const h = scr.h.p, *const d = scr.d.p;
    hipStream_t s = scr.s;
    hipError_t e = hipSuccess;
    if (after) {   // the handle's keypoint table may still be in flight on the handle's stream
        e = hipEventRecord(scr.ev[2], after);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, scr.ev[2], 0);
    }
    if (e == hipSuccess) e = msorb::small_copy(d, h, in_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[0], s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kernel, dim3(n_problems), dim3(kThreads), 0, s, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[1], s);
    if (e == hipSuccess) e = msorb::small_copy(h + o_res, d + o_res, o_end - o_res, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && elapsed_ms) e = hipEventElapsedTime(elapsed_ms, scr.ev[0], scr.ev[1]);
    if (e != hipSuccess) return hip_fail(scr, "pose_optimization", e);
    return MSORB_OK;
}

int run_staged(ThreadScratch& scr, const Staged& L, const KpLite* d_kp, const float* level_inv_sigma2, int nlevels, hipStream_t after,
               float* elapsed_ms) {
    uint8_t* const d = scr.d.p;
    PoseArgs A{};
    A.prob = reinterpret_cast<const PoseProblemDev*>(d + L.o_prob);
    if (L.frame) {
        A.kp = d_kp;
        A.kp_idx = reinterpret_cast<const int*>(d + L.o_a);
        for (int l = 0; l < MSORB_MAX_LEVELS; l++) A.level_inv_sigma2[l] = l < nlevels ? level_inv_sigma2[l] : 0.0f;
    } else {
        A.xy = reinterpret_cast<const float*>(d + L.o_a);
        A.u_right = reinterpret_cast<const float*>(d + L.o_ur);
        A.inv_sigma2 = reinterpret_cast<const float*>(d + L.o_inv);
    }
    A.delta_mono = (float)std::sqrt(5.991);
    A.delta_stereo = (float)std::sqrt(7.815);
    A.pos_w = reinterpret_cast<const float*>(d + L.o_pos);
    A.result = reinterpret_cast<msorb_pose_result*>(d + L.o_res);
    A.outlier = d + L.o_out;
    A.chi2_ws = reinterpret_cast<double*>(d + L.o_ws);
    return launch_staged(scr, pose_opt_kernel, A, L.n_problems, L.in_bytes, L.o_res, L.o_ws, after, elapsed_ms);
}

}  // namespace

extern "C" int msorb_pose_optimization_capacity(void) { return kResident; }

extern "C" int msorb_pose_optimization_batch(int device, int n_problems, const msorb_pose_problem* problems, const int* obs_offset,
                                             const float* xy, const float* u_right, const float* inv_sigma2, const float* pos_w,
                                             uint8_t* outlier_out, msorb_pose_result* results, float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (n_problems < 0 || (n_problems > 0 && (!problems || !obs_offset || !results))) return MSORB_E_INVALID;
    if (n_problems == 0) return MSORB_OK;
    bool strided = false;
    if (obs_offset[0] != 0) { set_last_error("pose_optimization_batch: obs_offset[0] must be 0"); return MSORB_E_INVALID; }
    for (int i = 0; i < n_problems; i++) {
        if (problems[i].n < 0 || obs_offset[i + 1] - obs_offset[i] != problems[i].n) {
            set_last_error("pose_optimization_batch: obs_offset does not match the problems' n");
            return MSORB_E_INVALID;
        }
        strided |= problems[i].n > kResident;
    }
    const size_t total = (size_t)obs_offset[n_problems];
    if (total > 0 && (!xy || !u_right || !inv_sigma2 || !pos_w || !outlier_out)) return MSORB_E_INVALID;
    if (int rc = msorb::require_device(device)) return rc;
    const Staged L(n_problems, total, false, strided);
    static thread_local ThreadScratch scr(true, 3);
    if (int rc = scr.acquire(device, L.dev_bytes, L.pin_bytes)) return rc;
    uint8_t* const h = scr.h.p;
    PoseProblemDev* hp = reinterpret_cast<PoseProblemDev*>(h + L.o_prob);
    for (int i = 0; i < n_problems; i++) { hp[i].p = problems[i]; hp[i].obs0 = obs_offset[i]; }
    if (total) {
        std::memcpy(h + L.o_a, xy, total * 8);
        std::memcpy(h + L.o_ur, u_right, total * 4);
        std::memcpy(h + L.o_inv, inv_sigma2, total * 4);
        std::memcpy(h + L.o_pos, pos_w, total * 12);
    }
    if (int rc = run_staged(scr, L, nullptr, nullptr, 0, nullptr, elapsed_ms)) return rc;
    std::memcpy(results, h + L.o_res, (size_t)n_problems * sizeof(msorb_pose_result));
    if (total) std::memcpy(outlier_out, h + L.o_out, total);
    return MSORB_OK;
}

extern "C" int msorb_frame_pose_optimization(msorb_frame* f, const msorb_pose_problem* p, const uint8_t* has_point, const float* pos_w,
                                             const float* inv_level_sigma2, int nlevels, uint8_t* outlier, msorb_pose_result* r) {
    if (!f || !p || !r || !inv_level_sigma2 || nlevels < 1 || nlevels > MSORB_MAX_LEVELS) return MSORB_E_INVALID;
    const int N = f->N;
    if (N > 0 && (!has_point || !pos_w || !outlier)) return MSORB_E_INVALID;
    size_t m = 0;
    for (int i = 0; i < N; i++) m += has_point[i] != 0;
    const Staged L(1, m, true, m > (size_t)kResident);
    static thread_local ThreadScratch scr(true, 3);
    if (int rc = scr.acquire(f->device, L.dev_bytes, L.pin_bytes)) return rc;
    uint8_t* const h = scr.h.p;
    PoseProblemDev* hp = reinterpret_cast<PoseProblemDev*>(h + L.o_prob);
    hp->p = *p;
    hp->p.n = (int)m;
    hp->obs0 = 0;
    int* idx = reinterpret_cast<int*>(h + L.o_a);
    float* pos = reinterpret_cast<float*>(h + L.o_pos);
    for (int i = 0, k = 0; i < N; i++)
        if (has_point[i]) {
            idx[k] = i;
            std::memcpy(pos + 3 * (size_t)k, pos_w + 3 * (size_t)i, 12);
            k++;
        }
    if (int rc = run_staged(scr, L, f->d_kp.p, inv_level_sigma2, nlevels, f->stream, nullptr)) return rc;
    std::memcpy(r, h + L.o_res, sizeof(msorb_pose_result));
    const uint8_t* out = h + L.o_out;
    for (size_t k = 0; k < m; k++) outlier[idx[k]] = out[k];
    return MSORB_OK;
}

// ---- the two-camera arm and the non-pinhole one-camera frame (RigModel)
extern "C" int msorb_pose_optimization_rig_capacity(void) { return kRigPerThread * kThreads; }

extern "C" int msorb_pose_optimization_rig_batch(int device, int n_problems, const msorb_pose_rig_problem* problems, const int* obs_offset,
                                                 const float* xy, const uint8_t* camera, const float* inv_sigma2, const float* pos_w,
                                                 uint8_t* outlier_out, msorb_pose_result* results, float* elapsed_ms) {
    if (elapsed_ms) *elapsed_ms = 0;
    if (n_problems < 0 || (n_problems > 0 && (!problems || !obs_offset || !results))) return MSORB_E_INVALID;
    if (n_problems == 0) return MSORB_OK;
    bool strided = false;
    if (obs_offset[0] != 0) { set_last_error("pose_optimization_rig_batch: obs_offset[0] must be 0"); return MSORB_E_INVALID; }
    for (int i = 0; i < n_problems; i++) {
        const msorb_pose_rig_problem& p = problems[i];
        if (p.n < 0 || obs_offset[i + 1] - obs_offset[i] != p.n) {
            set_last_error("pose_optimization_rig_batch: obs_offset does not match the problems' n");
            return MSORB_E_INVALID;
        }
        if (p.n_cameras != 1 && p.n_cameras != 2) { set_last_error("pose_optimization_rig_batch: n_cameras must be 1 or 2"); return MSORB_E_INVALID; }
        for (int c = 0; c < p.n_cameras; c++)
            if (p.cam[c].type != msorb::rig::kPinhole && p.cam[c].type != msorb::rig::kKannalaBrandt8) {
                set_last_error("pose_optimization_rig_batch: unknown camera type");
                return MSORB_E_INVALID;
            }
        strided |= p.n > kRigPerThread * kThreads;
    }
    const size_t total = (size_t)obs_offset[n_problems];
    if (total > 0 && (!xy || !camera || !inv_sigma2 || !pos_w || !outlier_out)) return MSORB_E_INVALID;
    for (int i = 0; i < n_problems; i++)
        for (int k = obs_offset[i]; k < obs_offset[i + 1]; k++)
            if (camera[k] >= problems[i].n_cameras) {
                set_last_error("pose_optimization_rig_batch: an observation names a camera the problem does not have");
                return MSORB_E_INVALID;
            }
    if (int rc = msorb::require_device(device)) return rc;
    // staging: [problems | xy | camera | inv_sigma2 | pos_w] up, [results | outlier] down, then the chi2 workspace of the strided problems
    const size_t o_xy = up16((size_t)n_problems * sizeof(RigProblemDev)), o_cam = o_xy + up16(total * 8), o_inv = o_cam + up16(total);
    const size_t o_pos = o_inv + up16(total * 4), in_bytes = o_pos + up16(total * 12);
    const size_t o_res = in_bytes, o_out = o_res + up16((size_t)n_problems * sizeof(msorb_pose_result)), o_ws = o_out + up16(total);
    static thread_local ThreadScratch scr(true, 3);
    if (int rc = scr.acquire(device, o_ws + (strided ? total * 8 : 0), o_ws)) return rc;
    uint8_t *const h = scr.h.p, *const d = scr.d.p;
    RigProblemDev* hp = reinterpret_cast<RigProblemDev*>(h);
    for (int i = 0; i < n_problems; i++) { hp[i].p = problems[i]; hp[i].obs0 = obs_offset[i]; }
    if (total) {
        std::memcpy(h + o_xy, xy, total * 8);
        std::memcpy(h + o_cam, camera, total);
        std::memcpy(h + o_inv, inv_sigma2, total * 4);
        std::memcpy(h + o_pos, pos_w, total * 12);
    }
    RigArgs A{};
    A.prob = reinterpret_cast<const RigProblemDev*>(d);
    A.xy = reinterpret_cast<const float*>(d + o_xy);
    A.camera = d + o_cam;
    A.inv_sigma2 = reinterpret_cast<const float*>(d + o_inv);
    A.pos_w = reinterpret_cast<const float*>(d + o_pos);
    A.delta_mono = (float)std::sqrt(5.991);
    A.delta_stereo = (float)std::sqrt(7.815);
    A.result = reinterpret_cast<msorb_pose_result*>(d + o_res);
    A.outlier = d + o_out;
    A.chi2_ws = reinterpret_cast<double*>(d + o_ws);
    if (int rc = launch_staged(scr, pose_opt_rig_kernel, A, n_problems, in_bytes, o_res, o_ws, nullptr, elapsed_ms)) return rc;
    std::memcpy(results, h + o_res, (size_t)n_problems * sizeof(msorb_pose_result));
    if (total) std::memcpy(outlier_out, h + o_out, total);
    return MSORB_OK;
}
