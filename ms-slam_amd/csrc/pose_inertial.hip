// Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame (src/Optimizer.cc:4422-4779, :4781-5172) for pinhole mono / stereo
// frames without a second camera: the four rounds of Gauss-Newton, the classifications, the recovery arm and the final Hessian in
// ONE launch, in double like g2o.  The arithmetic is pose_inertial_device.h, the same text a host compiler reads; this file is the
// executor that spreads it over a workgroup, the two stores of the visual edges, and the entries.
//
// One workgroup of 256 threads owns a problem (blockIdx.x = problem), as in pose_opt.hip.  Thread t owns the observations t,
// t + 256, ...: up to kPerThread = 8 of them live in registers as the reference's floats (n <= kResident = 2048); a longer problem
// walks the same indices in global memory, with the per-edge state (the stale chi2, the level) in a workspace.  Both add in the same
// order.  A pass maps the active visual edges to the 21 + 6 sums of the pose block and reduces them in section 9's order (thread
// ascending, xor butterfly 32..1, wavefronts 0..3 through a double-buffered LDS block); the inertial, random-walk and prior edges
// and the 15 or 30 unknowns' L D L^T live in LDS, one thread per entry.  No atomics: two runs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/msorb.h"
#include "hip_host.h"
#include "matcher_host.h"
#include "pose_inertial_device.h"

namespace msorb {
hipError_t small_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s);   // orb_kernels.hip
}
using msorb::KpLite;
using msorb::set_last_error;
using msorb::ThreadScratch;
using msorb::up16;
using namespace msorb::pinert;

namespace {

constexpr int kThreads = 256, kPerThread = 8, kResident = kThreads * kPerThread, kWaves = kThreads / 64;

static_assert(sizeof(msorb_pose_inertial_state) == 168 && sizeof(msorb_pose_inertial_problem) == 3632 &&
                  sizeof(msorb_pose_inertial_result) == 9272,
              "the records of include/msorb.h as the Python mirror lays them out");

struct PiArgs {
    const msorb_pose_inertial_problem* prob;
    const int* obs0;       // first observation of each problem in the flat arrays
    // flat form: per observation
    const float* xy;
    const float* u_right;
    const float* inv_sigma2;
    // frame form: the handle's keypoint table, the indices of the keypoints that have a point (ascending), mvInvLevelSigma2
    const KpLite* kp;
    const int* kp_idx;
    float level_inv_sigma2[MSORB_MAX_LEVELS];
    const float* pos_w;
    const uint8_t* close;
    double* chi2_ws;       // per observation, read and written by the problems with n > kResident only
    uint8_t* outlier;      // per observation: out (and the level of the strided form between the rounds)
    msorb_pose_inertial_result* result;
};

__device__ inline Ob load_ob(const PiArgs& A, int i) {
    Ob o;
    if (A.kp) {
        const KpLite kp = A.kp[A.kp_idx[i]];
        o.x = kp.x; o.y = kp.y; o.ur = kp.u_right;
        o.w = A.level_inv_sigma2[min(max(kp.octave, 0), MSORB_MAX_LEVELS - 1)];
    } else {
        o.x = A.xy[2 * (size_t)i]; o.y = A.xy[2 * (size_t)i + 1]; o.ur = A.u_right[i]; o.w = A.inv_sigma2[i];
    }
    o.X = A.pos_w[3 * (size_t)i]; o.Y = A.pos_w[3 * (size_t)i + 1]; o.Z = A.pos_w[3 * (size_t)i + 2];
    o.close = A.close[i] != 0;
    return o;
}

struct BlockExec {
    double* const lds;   // 2 blocks of kWaves * kSums
    int buf = 0;
    __device__ explicit BlockExec(double* l) : lds(l) {}
    __device__ inline int tid() const { return threadIdx.x; }
    __device__ inline int stride() const { return kThreads; }
    __device__ inline void barrier() { __syncthreads(); }
    __device__ inline bool leads(int k) const { return (int)threadIdx.x == 64 * k; }
    // block_sum of pose_opt.hip: every thread returns with the same bits; the two LDS blocks alternate, so the one barrier also
    // protects the block of the reduction before the last
    __device__ inline void sum(double* v, int n) {
        double* l = lds + (buf ^= 1) * kWaves * kSums;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
            for (int i = 0; i < kSums; i++)
                if (i < n) v[i] += msorb::se3::shfl_xor_f64(v[i], off);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0)
#pragma unroll
            for (int i = 0; i < kSums; i++)
                if (i < n) l[wave * kSums + i] = v[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kSums; i++)
            if (i < n) {
                double s = l[i];
                for (int w = 1; w < kWaves; w++) s += l[w * kSums + i];
                v[i] = s;
            }
    }
};

// the visual edges in registers
struct ResidentObs {
    Ob ob[kPerThread];
    double chi2[kPerThread];
    uint8_t level[kPerThread];
    int n;
    __device__ ResidentObs(const PiArgs& A, int obs0, int n_) : n(n_) {
#pragma unroll
        for (int k = 0; k < kPerThread; k++) {
            const int i = threadIdx.x + k * kThreads;
            ob[k] = i < n ? load_ob(A, obs0 + i) : Ob{};
            chi2[k] = 0;
            level[k] = 0;
        }
    }
    template <typename F>
    __device__ inline void each(F f) {
#pragma unroll
        for (int k = 0; k < kPerThread; k++)
            if ((int)threadIdx.x + k * kThreads < n) f(ob[k], chi2[k], level[k], (int)threadIdx.x + k * kThreads);
    }
};

// the visual edges in global memory, their state in the workspace
struct StridedObs {
    const PiArgs& A;
    int obs0, n;
    __device__ StridedObs(const PiArgs& a, int o, int n_) : A(a), obs0(o), n(n_) {
        for (int i = threadIdx.x; i < n; i += kThreads) { A.chi2_ws[obs0 + i] = 0; A.outlier[obs0 + i] = 0; }
    }
    template <typename F>
    __device__ inline void each(F f) {
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const Ob o = load_ob(A, obs0 + i);
            double chi2 = A.chi2_ws[obs0 + i];
            uint8_t level = A.outlier[obs0 + i];
            f(o, chi2, level, i);
            A.chi2_ws[obs0 + i] = chi2;
            A.outlier[obs0 + i] = level;
        }
    }
};

__global__ __launch_bounds__(kThreads) void pose_inertial_kernel(const PiArgs A) {
    __shared__ double lds[2 * kWaves * kSums];
    __shared__ Shared S;
    BlockExec ex(lds);
    const msorb_pose_inertial_problem& P = A.prob[blockIdx.x];
    const int n = P.n, obs0 = A.obs0[blockIdx.x];
    msorb_pose_inertial_result& R = A.result[blockIdx.x];
    uint8_t* flags = A.outlier + obs0;
    if (n <= kResident) {
        ResidentObs obs(A, obs0, n);
        if (P.form == 1) optimize<1>(ex, obs, P, S, flags, R);
        else optimize<0>(ex, obs, P, S, flags, R);
    } else {
        StridedObs obs(A, obs0, n);
        if (P.form == 1) optimize<1>(ex, obs, P, S, flags, R);
        else optimize<0>(ex, obs, P, S, flags, R);
    }
}

// One upload, one launch, one read-back on the calling thread's scratch.  Staging: [problems | obs0 | idx or (xy | u_right |
// inv_sigma2) | pos_w | close] up, [results | outlier] down, then the chi2 workspace of the problems above kResident.
struct Staged {
    int n_problems;
    size_t total;   // observations
    bool frame;
    size_t o_prob, o_obs0, o_a, o_ur, o_inv, o_pos, o_close, in_bytes, o_res, o_out, o_ws, dev_bytes, pin_bytes;
    Staged(int np, size_t tot, bool fr, bool strided) : n_problems(np), total(tot), frame(fr) {
        o_prob = 0;
        o_obs0 = up16((size_t)np * sizeof(msorb_pose_inertial_problem));
        o_a = o_obs0 + up16((size_t)np * 4);
        if (fr) { o_ur = o_inv = o_a; o_pos = o_a + up16(tot * 4); }
        else { o_ur = o_a + up16(tot * 8); o_inv = o_ur + up16(tot * 4); o_pos = o_inv + up16(tot * 4); }
        o_close = o_pos + up16(tot * 12);
        in_bytes = o_close + up16(tot);
        o_res = in_bytes;
        o_out = o_res + up16((size_t)np * sizeof(msorb_pose_inertial_result));
        o_ws = o_out + up16(tot);
        pin_bytes = o_ws;
        dev_bytes = o_ws + (strided ? tot * 8 : 0);
    }
};

int run_staged(ThreadScratch& scr, const Staged& L, const KpLite* d_kp, const float* level_inv_sigma2, int nlevels, hipStream_t after,
               float* elapsed_ms) {
    uint8_t *const h = scr.h.p, *const d = scr.d.p;
    hipStream_t s = scr.s;
    PiArgs A{};
    A.prob = reinterpret_cast<const msorb_pose_inertial_problem*>(d + L.o_prob);
    A.obs0 = reinterpret_cast<const int*>(d + L.o_obs0);
    if (L.frame) {
        A.kp = d_kp;
        A.kp_idx = reinterpret_cast<const int*>(d + L.o_a);
        for (int l = 0; l < MSORB_MAX_LEVELS; l++) A.level_inv_sigma2[l] = l < nlevels ? level_inv_sigma2[l] : 0.0f;
    } else {
        A.xy = reinterpret_cast<const float*>(d + L.o_a);
        A.u_right = reinterpret_cast<const float*>(d + L.o_ur);
        A.inv_sigma2 = reinterpret_cast<const float*>(d + L.o_inv);
    }
    A.pos_w = reinterpret_cast<const float*>(d + L.o_pos);
    A.close = d + L.o_close;
    A.result = reinterpret_cast<msorb_pose_inertial_result*>(d + L.o_res);
    A.outlier = d + L.o_out;
    A.chi2_ws = reinterpret_cast<double*>(d + L.o_ws);
    hipError_t e = hipSuccess;
    if (after) {   // the handle's keypoint table may still be in flight on the handle's stream
        e = hipEventRecord(scr.ev[2], after);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, scr.ev[2], 0);
    }
    if (e == hipSuccess) e = msorb::small_copy(d, h, L.in_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[0], s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pose_inertial_kernel, dim3(L.n_problems), dim3(kThreads), 0, s, A);
        e = hipGetLastError();
    }
    if (e == hipSuccess && elapsed_ms) e = hipEventRecord(scr.ev[1], s);
    if (e == hipSuccess) e = msorb::small_copy(h + L.o_res, d + L.o_res, L.o_ws - L.o_res, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && elapsed_ms) e = hipEventElapsedTime(elapsed_ms, scr.ev[0], scr.ev[1]);
    if (e != hipSuccess) {
        set_last_error(std::string("pose_inertial_optimization: ") + hipGetErrorString(e));
        scr.release();
        return MSORB_E_HIP;
    }
    return MSORB_OK;
}

bool finite_all(const double* p, int n) {
    for (int i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}
bool finite_all(const float* p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// the refusals that depend on one problem record alone; nullptr = accepted
const char* problem_refusal(const msorb_pose_inertial_problem& p) {
    if (p.form != 0 && p.form != 1) return "an unknown form (0 = last KeyFrame, 1 = last frame)";
    if (p.n < 0) return "a negative number of observations";
    if (!finite_all(p.frame.Rwb, 21) || !finite_all(p.other.Rwb, 21) || !finite_all(p.Rcw, 27) || !finite_all(&p.fx, (size_t)5) ||
        !finite_all(p.pre.dR, (size_t)67) || !finite_all(p.pre.info, 81) || !finite_all(p.info_gyro, 18))
        return "a non-finite value in a problem";
    if (p.form == 1 && (!finite_all(p.prior.Rwb, 21) || !finite_all(p.H, 225))) return "a non-finite value in the prior";
    return nullptr;
}

int refuse(const char* entry, const char* what) {
    set_last_error(std::string(entry) + ": " + what);
    return MSORB_E_INVALID;
}

}  // namespace

extern "C" int msorb_pose_inertial_optimization_capacity(void) { return kResident; }

extern "C" int msorb_pose_inertial_optimization_batch(int device, int n_problems, const msorb_pose_inertial_problem* problems,
                                                      const int* obs_offset, const float* xy, const float* u_right,
                                                      const float* inv_sigma2, const float* pos_w, const uint8_t* close,
                                                      uint8_t* outlier_out, msorb_pose_inertial_result* results, float* elapsed_ms) {
    static const char* const kEntry = "pose_inertial_optimization_batch";
    if (n_problems < 0) return refuse(kEntry, "a negative number of problems");
    if (n_problems > 0 && (!problems || !obs_offset || !results)) return refuse(kEntry, "a null required pointer");
    if (n_problems == 0) { if (elapsed_ms) *elapsed_ms = 0; return MSORB_OK; }
    bool strided = false;
    if (obs_offset[0] != 0) return refuse(kEntry, "obs_offset[0] must be 0");
    for (int i = 0; i < n_problems; i++) {
        if (const char* why = problem_refusal(problems[i])) return refuse(kEntry, why);
        if (obs_offset[i + 1] - obs_offset[i] != problems[i].n) return refuse(kEntry, "obs_offset does not match the problems' n");
        strided |= problems[i].n > kResident;
    }
    const size_t total = (size_t)obs_offset[n_problems];
    if (total > 0 && (!xy || !u_right || !inv_sigma2 || !pos_w || !close || !outlier_out)) return refuse(kEntry, "a null required pointer");
    if (!finite_all(xy, 2 * total) || !finite_all(u_right, total) || !finite_all(inv_sigma2, total) || !finite_all(pos_w, 3 * total))
        return refuse(kEntry, "a non-finite value in an observation");
    if (int rc = msorb::require_device(device)) return rc;
    const Staged L(n_problems, total, false, strided);
    static thread_local ThreadScratch scr(true, 3);
    if (int rc = scr.acquire(device, L.dev_bytes, L.pin_bytes)) return rc;
    uint8_t* const h = scr.h.p;
    std::memcpy(h + L.o_prob, problems, (size_t)n_problems * sizeof(*problems));
    std::memcpy(h + L.o_obs0, obs_offset, (size_t)n_problems * 4);
    if (total) {
        std::memcpy(h + L.o_a, xy, total * 8);
        std::memcpy(h + L.o_ur, u_right, total * 4);
        std::memcpy(h + L.o_inv, inv_sigma2, total * 4);
        std::memcpy(h + L.o_pos, pos_w, total * 12);
        std::memcpy(h + L.o_close, close, total);
    }
    float ms = 0;
    if (int rc = run_staged(scr, L, nullptr, nullptr, 0, nullptr, elapsed_ms ? &ms : nullptr)) return rc;
    std::memcpy(results, h + L.o_res, (size_t)n_problems * sizeof(msorb_pose_inertial_result));
    for (int i = 0; i < n_problems; i++) finish_prior(problems[i].form, results[i]);
    if (total) std::memcpy(outlier_out, h + L.o_out, total);
    if (elapsed_ms) *elapsed_ms = ms;
    return MSORB_OK;
}

extern "C" int msorb_frame_pose_inertial_optimization(msorb_frame* f, const msorb_pose_inertial_problem* p, const uint8_t* has_point,
                                                      const float* pos_w, const uint8_t* close, const float* inv_level_sigma2,
                                                      int nlevels, uint8_t* outlier, msorb_pose_inertial_result* r) {
    static const char* const kEntry = "frame_pose_inertial_optimization";
    if (!f || !p || !r || !inv_level_sigma2) return refuse(kEntry, "a null required pointer");
    if (nlevels < 1 || nlevels > MSORB_MAX_LEVELS) return refuse(kEntry, "nlevels out of range");
    const int N = f->N;
    if (N > 0 && (!has_point || !pos_w || !close || !outlier)) return refuse(kEntry, "a null required pointer");
    msorb_pose_inertial_problem q = *p;
    size_t m = 0;
    for (int i = 0; i < N; i++) m += has_point[i] != 0;
    q.n = (int)m;
    if (const char* why = problem_refusal(q)) return refuse(kEntry, why);
    if (!finite_all(inv_level_sigma2, (size_t)nlevels)) return refuse(kEntry, "a non-finite value in inv_level_sigma2");
    for (int i = 0; i < N; i++)
        if (has_point[i] && !finite_all(pos_w + 3 * (size_t)i, (size_t)3)) return refuse(kEntry, "a non-finite value in an observation");
    const Staged L(1, m, true, m > (size_t)kResident);
    static thread_local ThreadScratch scr(true, 3);
    if (int rc = scr.acquire(f->device, L.dev_bytes, L.pin_bytes)) return rc;
    uint8_t* const h = scr.h.p;
    std::memcpy(h + L.o_prob, &q, sizeof(q));
    *reinterpret_cast<int*>(h + L.o_obs0) = 0;
    int* idx = reinterpret_cast<int*>(h + L.o_a);
    float* pos = reinterpret_cast<float*>(h + L.o_pos);
    uint8_t* cl = h + L.o_close;
    for (int i = 0, k = 0; i < N; i++)
        if (has_point[i]) {
            idx[k] = i;
            std::memcpy(pos + 3 * (size_t)k, pos_w + 3 * (size_t)i, 12);
            cl[k] = close[i];
            k++;
        }
    if (int rc = run_staged(scr, L, f->d_kp.p, inv_level_sigma2, nlevels, f->stream, nullptr)) return rc;
    std::memcpy(r, h + L.o_res, sizeof(*r));
    finish_prior(q.form, *r);
    const uint8_t* out = h + L.o_out;
    for (size_t k = 0; k < m; k++) outlier[idx[k]] = out[k];
    return MSORB_OK;
}
